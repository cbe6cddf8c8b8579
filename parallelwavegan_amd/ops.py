"""Tensor-level wrappers over the C ABI (device pointers in, device pointers out).

PyTorch is used here only as the owner of device memory and streams.
"""
import ctypes

import torch

from . import _lib
from ._lib import ConvDesc, ResUnitDesc, WaveNetDesc

ACT = {None: _lib.PWG_ACT_NONE, "none": _lib.PWG_ACT_NONE, "leaky_relu": _lib.PWG_ACT_LEAKY_RELU,
       "tanh": _lib.PWG_ACT_TANH, "relu": _lib.PWG_ACT_RELU}
PAD = {"zero": _lib.PWG_PAD_ZERO, "reflect": _lib.PWG_PAD_REFLECT, "replicate": _lib.PWG_PAD_REPLICATE}


# The staleness rule of every derived weight image: an image is current
# while cache_epoch() and the tensor_state() of every tensor it was derived from are what they were when it was built.
PARAM_EPOCH = [0]


def bump_param_epoch():
    """Invalidate every cached weight image (e.g. before a hipGraph capture, so that all weight
    preparation kernels of the captured step are recorded inside the graph)."""
    PARAM_EPOCH[0] += 1


def cache_epoch():
    """The global part of the key: what ``bump_param_epoch`` bumps."""
    return PARAM_EPOCH[0]


def param_epoch(p):
    """The engine's own update count of ``p``: parameters updated through raw pointers (fused optimizer kernels) do not
    bump torch's version counter; ``bump_params`` bumps this instead."""
    return getattr(p, "_pwg_epoch", 0)


def tensor_state(t):
    """The per-tensor part of the key: storage address, torch's version counter, the engine's epoch, device."""
    return (t.data_ptr(), tensor_version(t), param_epoch(t), t.device)


def tensor_version(t):
    """torch's version counter of ``t``.  Tensors created or loaded under ``torch.inference_mode()`` track none (reading
    it raises) and cannot be written in place outside inference mode either: a constant stands in."""
    return -1 if t.is_inference() else t._version


def bump_params(params):
    """Mark parameters as changed through raw pointers (fused optimizer kernels)."""
    for p in params:
        p._pwg_epoch = getattr(p, "_pwg_epoch", 0) + 1


# Data-parallel gradient slots (distributed.GradReducer): parameter storage address -> [bucket view, weak reference to
# the owner, claim epoch] (the owner drops its entries in remove() and, through weakref.finalize, when it is collected).
# Contract: like ``.grad`` itself, a slot ACCUMULATES every contribution between two ``prepare()`` calls -- a second
# backward() over a retained graph adds to it, as AccumulateGrad would -- and a node writes its parameters' slots
# whenever it runs, so the ``inputs=``-restricted backward calls of one pass must cover disjoint sub-networks (the
# trainer's exchange groups are the independent sub-discriminators).
# A weight-gradient launch whose layer's parameter has a free slot writes its result straight into the bucket:
# autograd's AccumulateGrad adopts the returned alias as ``p.grad`` without a copy and the reducer's hook finds nothing
# left to copy.  A slot is claimed once per backward pass (the owner's epoch); later contributions of the same pass --
# the discriminator phase differentiates D(y) and D(G(c)) in one pass -- are added into the slot by their own node.
GRAD_SLOTS = {}


def claim_grad_slots(keys_shapes):
    """Claim the gradient slots of one layer's parameters together.  ``keys_shapes``: [(parameter address, shape)].
    Returns ``(aliases, accumulate)`` or ``(None, False)`` when any of them has no slot (then nothing is claimed):
    the FIRST claim of a backward pass gets ``accumulate = False`` -- the caller's kernels write the slots and the
    aliases go back to autograd as the gradients; a later claim of the same pass gets ``accumulate = True`` -- the
    caller adds its contribution INTO the slots (same stream, program order) and returns None to autograd, which then
    neither sums nor copies anything."""
    entries = []
    for key, shape in keys_shapes:
        e = GRAD_SLOTS.get(key)
        owner = e[1]() if e is not None else None  # (weak: a dropped reducer must not be kept alive by this table)
        if e is not None and owner is None:
            del GRAD_SLOTS[key]
        if owner is None or not owner.enabled or not owner.direct_slots or e[0].numel() != _numel(shape):
            return None, False
        entries.append((e, shape, owner))
    states = {e[2] == owner.epoch for e, _, owner in entries}
    if len(states) != 1:  # (cannot happen while a layer's parameters live in one reducer; stay on the copying path)
        return None, False
    later = states.pop()
    cur = torch.cuda.current_stream(entries[0][0][0].device) if entries[0][0][0].is_cuda else None
    for e, _, owner in entries:
        e[2] = owner.epoch
        if not later:  # remember where this pass's first contribution is written (see slot_add)
            if len(e) > 3:
                e[3] = cur
            else:
                e.append(cur)
    if later:
        first = entries[0][0][3] if len(entries[0][0]) > 3 else None
        later = first if first is not None else True
    return [e[0].view(shape) for e, shape, _ in entries], later


def slot_add(slot_view, contribution, later):
    """Add a LATER contribution of one backward pass into a gradient slot.  ``later`` is what :func:`claim_grad_slots`
    returned: True, or the stream the pass's FIRST contribution was written on.  The two passes of a layer normally run
    on one stream (program order).  They do not when one of them is the un-forked re-evaluation of a stateful
    sub-discriminator (``only=[...]`` with a single branch: caller's stream) and the other one the forked full pass (side
    stream): an ``add_`` on the caller's stream was then unordered against the first write -- and against the reducer
    hook's event, which autograd places on the first write's stream (round 6: the bias gradients of HiFi-GAN's spectrally
    normalised scale discriminator; found through the eager fork, profiles/r06_eager_nan_bisect.txt; the captured graph
    had the same two unordered nodes).  The addition is issued on the FIRST stream, after this stream's producer."""
    t = contribution.reshape(slot_view.shape)
    if later is True or not t.is_cuda:
        slot_view.add_(t)
        return
    cur = torch.cuda.current_stream(t.device)
    if later == cur:
        slot_view.add_(t)
        return
    done = torch.cuda.Event()
    done.record(cur)
    later.wait_event(done)
    with torch.cuda.stream(later):
        slot_view.add_(t)
    t.record_stream(later)


def _numel(shape):
    n = 1
    for d in shape:
        n *= int(d)
    return n


def _require_device(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "parallelwavegan_amd ops run only on an MI355X device tensor (got a CPU tensor); "
                "there is no CPU fallback path"
            )
        if t.dtype != torch.float32:
            raise RuntimeError(f"expected float32 tensor, got {t.dtype}")
        if not t.is_contiguous():
            raise RuntimeError("expected contiguous tensor")


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def make_conv_desc(batch, c_in, c_out, t_in, t_out, kernel, stride=1, dilation=1, pad_left=0, groups=1,
                   transposed=False, width=1, pad_mode="zero", pre_act=None, pre_slope=0.0, post_act=None,
                   post_slope=0.0, out_mul=1.0, out_div=1.0):
    return ConvDesc(batch, c_in, c_out, t_in, t_out, width, kernel, stride, dilation, pad_left, groups,
                    int(bool(transposed)), PAD[pad_mode], ACT[pre_act], float(pre_slope), ACT[post_act],
                    float(post_slope), float(out_mul), float(out_div))


def conv_out_length(t_in, kernel, stride=1, dilation=1, pad_left=0, pad_right=0):
    return (t_in + pad_left + pad_right - dilation * (kernel - 1) - 1) // stride + 1


def conv_transpose_out_length(t_in, kernel, stride, padding, output_padding):
    return (t_in - 1) * stride - 2 * padding + kernel + output_padding


def packed_weight_floats(desc):
    n = _lib.lib().pwg_conv1d_packed_weight_floats(ctypes.byref(desc))
    if n == 0:
        _lib.check(-1, "packed_weight_floats")
    return n


def pack_weight(desc, w, scale=None):
    """torch-layout weight (+ optional weight_norm row scale) -> packed image."""
    _require_device(w, scale)
    out = torch.empty(packed_weight_floats(desc), device=w.device, dtype=torch.float32)
    _lib.check(_lib.lib().pwg_conv1d_pack_weight(ctypes.byref(desc), _ptr(w), _ptr(scale), _ptr(out), _stream()),
               "conv1d_pack_weight")
    return out


def _workspace(n_floats, device):
    """Scratch for a split reduction (caller-owned per the C ABI: torch's caching allocator here)."""
    if not n_floats:
        return None, 0
    return torch.empty(n_floats, device=device, dtype=torch.float32), n_floats


def conv1d_forward(desc, x, w_packed, bias=None, add1=None, add2=None, out=None):
    _require_device(x, w_packed, bias, add1, add2, out)
    if out is None:
        out = torch.empty((desc.batch, desc.c_out, desc.t_out * desc.width), device=x.device, dtype=torch.float32)
    assert x.numel() == desc.batch * desc.c_in * desc.t_in * desc.width, (tuple(x.shape), desc.batch, desc.c_in, desc.t_in)
    assert out.numel() == desc.batch * desc.c_out * desc.t_out * desc.width
    ws, ws_n = _workspace(_lib.lib().pwg_conv1d_forward_workspace_floats(ctypes.byref(desc)), x.device)
    _lib.check(_lib.lib().pwg_conv1d_forward(ctypes.byref(desc), _ptr(x), _ptr(w_packed), _ptr(bias), _ptr(add1),
                                             _ptr(add2), _ptr(out), _ptr(ws), ws_n, _stream()), "conv1d_forward")
    return out


def conv1d_bf16_supported(desc):
    """Does the bf16-operand inference kernel (csrc/conv1d_bf16.hip) cover this descriptor?  Host logic only (no
    device needed); ``_lib.lib().pwg_last_error()`` names the reason for a False."""
    return bool(_lib.lib().pwg_conv1d_bf16_supported(ctypes.byref(desc)))


def _zero_padded(desc):
    """``desc`` with zero padding: a weight image does not depend on padding, which the MFMA kernels' geometry check
    admits only as zero."""
    if desc.pad_mode == PAD["zero"]:
        return desc
    desc = ConvDesc.from_buffer_copy(desc)
    desc.pad_mode = PAD["zero"]
    return desc


def _pack_weight_mfma(kind, desc, w, scale, op="conv1d"):
    """The packer of the ``kind`` ("bf16" / "split") MFMA kernel: one image layout, csrc/mfma_conv.h.  ``op``: the
    entry-point family, "conv1d" or "convtr1d" (the split-operand transposed convolution)."""
    _require_device(w, scale)
    n = getattr(_lib.lib(), f"pwg_{op}_{kind}_packed_weight_bytes")(ctypes.byref(desc))
    if n == 0:
        _lib.check(-1, f"{op}_{kind}_packed_weight_bytes")
    out = torch.empty(n, device=w.device, dtype=torch.uint8)
    pack = getattr(_lib.lib(), f"pwg_{op}_{kind}_pack_weight")
    _lib.check(pack(ctypes.byref(desc), _ptr(w), _ptr(scale), _ptr(out), _stream()), f"{op}_{kind}_pack_weight")
    return out


def _conv1d_forward_mfma(kind, desc, image_desc, x, w_packed, bias, add1, add2, out, cfg, op="conv1d", entry="cfg"):
    """The forward of the ``kind`` ("bf16" / "split") MFMA kernel.  ``image_desc``: the descriptor the image was packed
    through; ``cfg``: the tuning integers of ``pwg_<op>_<kind>_forward_<entry>``, None for the default launch."""
    name = f"{op}_forward_{kind}"
    _require_device(x, bias, add1, add2, out)
    if not w_packed.is_cuda or w_packed.dtype != torch.uint8:
        raise RuntimeError(f"{name}: w_packed must be the device image of pack_weight_{kind}")
    if out is None:
        out = torch.empty((desc.batch, desc.c_out, desc.t_out), device=x.device, dtype=torch.float32)
    assert x.numel() == desc.batch * desc.c_in * desc.t_in, (tuple(x.shape), desc.batch, desc.c_in, desc.t_in)
    assert out.numel() == desc.batch * desc.c_out * desc.t_out
    image_bytes = getattr(_lib.lib(), f"pwg_{op}_{kind}_packed_weight_bytes")(ctypes.byref(image_desc))
    if image_bytes == 0:  # the kernel refuses the descriptor: report its reason, not a mismatch
        _lib.check(-1, f"{op}_{kind}_packed_weight_bytes")
    assert w_packed.numel() == image_bytes, f"{name}: w_packed is not this layer's {kind} image"
    for t in (add1, add2):
        assert t is None or t.numel() == out.numel()
    args = (ctypes.byref(desc), _ptr(x), _ptr(w_packed), _ptr(bias), _ptr(add1), _ptr(add2), _ptr(out))
    if cfg is None:
        rc = getattr(_lib.lib(), f"pwg_{op}_{kind}_forward")(*args, None, 0, _stream())
    else:
        rc = getattr(_lib.lib(), f"pwg_{op}_{kind}_forward_{entry}")(*args, *cfg, _stream())
    _lib.check(rc, name)
    return out


def pack_weight_bf16(desc, w, scale=None):
    """torch-layout fp32 weight (+ optional weight_norm row scale) -> bf16 MFMA weight image (an opaque byte tensor);
    the effective weight ``w * scale`` is rounded to bf16 here, once.  The image does not depend on padding, which the
    packer's geometry check admits only as zero: a reflect- / replicate-padded layer (the causal MelGAN layers, for
    the bf16 stream kernel) is packed through a descriptor of the same geometry with zero padding."""
    return _pack_weight_mfma("bf16", _zero_padded(desc), w, scale)


def conv1d_forward_bf16(desc, x, w_packed, bias=None, add1=None, add2=None, out=None, mfma_shape=None):
    """Fused convolution with bf16 operands and fp32 accumulation / epilogue (inference only).  ``mfma_shape``
    (tuning): 32 or 16 selects the MFMA instruction explicitly."""
    return _conv1d_forward_mfma("bf16", desc, _zero_padded(desc), x, w_packed, bias, add1, add2, out,
                                None if mfma_shape is None else (int(mfma_shape),))


def conv1d_split_supported(desc):
    """Does the split-operand inference kernel (csrc/conv1d_split.hip) cover this descriptor?  Host logic only (no
    device needed); ``_lib.lib().pwg_last_error()`` names the reason for a False."""
    return bool(_lib.lib().pwg_conv1d_split_supported(ctypes.byref(desc)))


def pack_weight_split(desc, w, scale=None):
    """torch-layout fp32 weight (+ optional weight_norm row scale) -> the three bf16 MFMA weight images of the
    split-operand kernel (an opaque byte tensor); the effective weight ``w * scale`` is split here, once."""
    return _pack_weight_mfma("split", desc, w, scale)


STEP_FORMS = {1: "resident", 2: "streamed"}


def conv1d_split_step_form(desc):
    """The form of the reduction step the split-operand kernel's launch plan chooses for this descriptor: "resident" or
    "streamed" (csrc/conv1d_split.hip, ``split_step_form``).  Host logic only (no device needed); an unsupported
    descriptor raises with the library's reason."""
    form = _lib.lib().pwg_conv1d_split_step_form(ctypes.byref(desc))
    if form == 0:
        _lib.check(-1, "conv1d_split_step_form")
    return STEP_FORMS[form]


WINDOW_FORMS = {1: "staged", 2: "prefetched"}


def conv1d_split_window_form(desc):
    """The form of the window staging the split-operand kernel's launch plan chooses for this descriptor: "staged" or
    "prefetched" (csrc/conv1d_split.hip, ``split_window_form``).  Host logic only (no device needed); an unsupported
    descriptor raises with the library's reason."""
    form = _lib.lib().pwg_conv1d_split_window_form(ctypes.byref(desc))
    if form == 0:
        _lib.check(-1, "conv1d_split_window_form")
    return WINDOW_FORMS[form]


def conv1d_forward_split(desc, x, w_packed, bias=None, add1=None, add2=None, out=None, mfma_shape=None, tile_mode=0,
                         step_form=0, window_form=0):
    """Fused fp32 convolution computed on the bf16 MFMA from 3-way split operands (inference only).
    ``mfma_shape`` (tuning): 32 or 16 selects the MFMA instruction; ``tile_mode`` (tests): 1 = full-size, 2 = half-size
    tiles instead of the small-grid rule; ``step_form`` (tests / A-B): 1 = the resident, 2 = the streamed reduction step
    instead of the plan's choice (same bits); ``window_form`` (tests / A-B): 1 = the staged, 2 = the prefetched window
    instead of the plan's choice (same bits)."""
    if window_form:
        cfg = (int(mfma_shape or 16), int(tile_mode), int(step_form), int(window_form))
        return _conv1d_forward_mfma("split", desc, desc, x, w_packed, bias, add1, add2, out, cfg, entry="window")
    if step_form:
        cfg = (int(mfma_shape or 16), int(tile_mode), int(step_form))
        return _conv1d_forward_mfma("split", desc, desc, x, w_packed, bias, add1, add2, out, cfg, entry="step")
    cfg = None if mfma_shape is None and not tile_mode else (int(mfma_shape or 16), int(tile_mode))
    return _conv1d_forward_mfma("split", desc, desc, x, w_packed, bias, add1, add2, out, cfg)


def convtr1d_split_supported(desc):
    """Does the split-operand transposed convolution (csrc/conv1d_split.hip, ``convtr1d_split_mfma_kernel``) cover this
    descriptor -- a ConvTranspose1d with kernel == 2 * stride?  Host logic only (no device needed);
    ``_lib.lib().pwg_last_error()`` names the reason for a False."""
    return bool(_lib.lib().pwg_convtr1d_split_supported(ctypes.byref(desc)))


def pack_weight_split_transposed(desc, w, scale=None):
    """torch-layout ConvTranspose1d weight (C_in, C_out, k) (+ optional weight_norm scale, per input channel) -> the
    three bf16 images of the split-operand transposed kernel: three parts of the bf16 kernel's transposed image."""
    return _pack_weight_mfma("split", desc, w, scale, op="convtr1d")


def conv1d_forward_split_transposed(desc, x, w_packed, bias=None, add1=None, add2=None, out=None, mfma_shape=None,
                                    tile_mode=0):
    """:func:`conv1d_forward_split` for a ConvTranspose1d with kernel == 2 * stride (inference only);
    ``mfma_shape`` / ``tile_mode`` as there."""
    cfg = None if mfma_shape is None and not tile_mode else (int(mfma_shape or 16), int(tile_mode))
    return _conv1d_forward_mfma("split", desc, desc, x, w_packed, bias, add1, add2, out, cfg, op="convtr1d")


def conv1d_stream_supported(desc):
    """Does the streaming kernel (csrc/conv1d_stream.hip) cover this descriptor -- a causal stride-1 convolution or the
    causal k = 2s transposed convolution, ``desc.t_in`` = columns per push?  Host logic only (no device needed);
    ``_lib.lib().pwg_last_error()`` names the reason for a False."""
    return bool(_lib.lib().pwg_conv1d_stream_supported(ctypes.byref(desc)))


def conv1d_stream_hist_floats(desc):
    """Floats of one history buffer of the layer: ``batch * c_in * H`` (0: unsupported, or a layer without history)."""
    return _lib.lib().pwg_conv1d_stream_hist_floats(ctypes.byref(desc))


def conv1d_stream_plan(desc):
    """The tile and grid every conv stream launch of ``desc`` takes, in either precision and every form (host only: no
    launch, no device needed): dict(tile=(rows, columns), grid=(column tiles, row blocks, batch)).  An unsupported
    descriptor raises with the library's reason."""
    out = (ctypes.c_int32 * 5)()
    _lib.check(_lib.lib().pwg_conv1d_stream_plan(ctypes.byref(desc), out), "conv1d_stream_plan")
    return dict(tile=(out[0], out[1]), grid=(out[2], out[3], out[4]))


def _conv1d_stream_out(desc, x, hist_in, hist_out, add1, add2, out):
    """The checks the two conv stream wrappers share -> ``out`` (allocated if None)."""
    if out is None:
        out = torch.empty((desc.batch, desc.c_out, desc.t_out), device=x.device, dtype=torch.float32)
    assert x.numel() == desc.batch * desc.c_in * desc.t_in, (tuple(x.shape), desc.batch, desc.c_in, desc.t_in)
    assert out.numel() == desc.batch * desc.c_out * desc.t_out
    n_hist = conv1d_stream_hist_floats(desc)
    for t in (hist_in, hist_out):
        assert t is None or t.numel() == n_hist, (tuple(t.shape), n_hist)
    for t in (add1, add2):
        assert t is None or t.numel() == out.numel()
    return out


def conv1d_stream_forward(desc, x, hist_in, hist_out, w_packed, bias=None, add1=None, add2=None, out=None):
    """One chunk of a causal convolution's stream: ``out`` from the ``desc.t_in`` new columns ``x`` and the history
    ``hist_in`` (None: start of stream), and ``hist_out`` = the last H columns of ``concat(hist_in, x)``, in one
    launch.  ``hist_in`` and ``hist_out`` must be distinct buffers."""
    _require_device(x, hist_in, hist_out, w_packed, bias, add1, add2, out)
    out = _conv1d_stream_out(desc, x, hist_in, hist_out, add1, add2, out)
    _lib.check(_lib.lib().pwg_conv1d_stream_forward(ctypes.byref(desc), _ptr(x), _ptr(hist_in), _ptr(hist_out),
                                                    _ptr(w_packed), _ptr(bias), _ptr(add1), _ptr(add2), _ptr(out),
                                                    _stream()), "conv1d_stream_forward")
    return out


def conv1d_stream_delayed_supported(desc, delay1=0, delay2=0):
    """Does the delayed form of the streaming kernel cover this descriptor with addend delays of ``delay1`` / ``delay2``
    columns?  What :func:`conv1d_stream_supported` admits, with zero padding and delays up to the cap of a history.  Host
    logic only; ``_lib.lib().pwg_last_error()`` names the reason for a False."""
    return bool(_lib.lib().pwg_conv1d_stream_delayed_supported(ctypes.byref(desc), int(delay1), int(delay2)))


def conv1d_stream_delayed_forward(desc, x, hist_in, hist_out, w_packed, bias=None, add1=None, add1_hist=(None, None),
                                  delay1=0, add2=None, add2_hist=(None, None), delay2=0, valid=None, out=None):
    """:func:`conv1d_stream_forward` for a layer of a non-causal network streamed with a fixed look-ahead: addend ``i``
    is read through a delay line of ``delay_i`` columns -- ``add_i_hist = (hist_in, hist_out)``, each (batch, c_out,
    delay_i), ``hist_in`` None for zeros; ``hist_out`` receives the last ``delay_i`` columns of ``concat(hist_in,
    add_i)`` -- and output columns outside ``valid = (lo, hi)`` (chunk-relative; None: all of them are valid) are stored
    as exact zeros.  One launch."""
    _require_device(w_packed)
    return _conv1d_stream_delayed(_lib.lib().pwg_conv1d_stream_delayed_forward, "conv1d_stream_delayed_forward", desc, x, hist_in, hist_out, w_packed, bias, add1,
                                  add1_hist, delay1, add2, add2_hist, delay2, valid, out)


def _conv1d_stream_delayed(entry, name, desc, x, hist_in, hist_out, image, bias, add1, add1_hist, delay1, add2, add2_hist,
                           delay2, valid, out, slots=None):
    """What the delayed and slotted conv stream wrappers share: the checks of every tensor but the weight image, and the
    call of the library's ``entry``.  ``slots``: None for a delayed entry, which takes the window ``valid``; else
    ``(table, rate, delay)`` of a slotted one, which takes those in the window's place."""
    flat = (add1_hist[0], add1_hist[1], add2_hist[0], add2_hist[1])
    _require_device(x, hist_in, hist_out, bias, add1, add2, out, *flat)
    out = _conv1d_stream_out(desc, x, hist_in, hist_out, add1, add2, out)
    for delay, (h_in, h_out) in ((delay1, add1_hist), (delay2, add2_hist)):
        for t in (h_in, h_out):
            assert t is None or t.numel() == desc.batch * desc.c_out * delay, (tuple(t.shape), delay)
    if slots is None:
        lo, hi = (0, desc.t_out) if valid is None else valid
        position = (int(lo), int(hi))
    else:
        table, rate, delay = slots
        if table is None or not table.is_cuda or table.dtype != torch.int32 or not table.is_contiguous():
            raise RuntimeError(f"{name}: slots must be a contiguous int32 device tensor (the kernel reads it; there is no "
                               "CPU fallback path)")
        assert tuple(table.shape) == (desc.batch, SLOT_INTS), (tuple(table.shape), desc.batch)
        position = (_ptr(table), int(rate), int(delay))
    _lib.check(entry(
        ctypes.byref(desc), _ptr(x), _ptr(hist_in), _ptr(hist_out), _ptr(image), _ptr(bias),
        _ptr(add1), _ptr(flat[0]), _ptr(flat[1]), int(delay1), _ptr(add2), _ptr(flat[2]), _ptr(flat[3]), int(delay2),
        *position, _ptr(out), _stream()), name)
    return out


# A row of a slotted launch's table (include/pwg_kernels.h): [frames before, frames left, flags, 0]
SLOT_INTS = 4
SLOT_PAUSED, SLOT_LEFT_KNOWN = 1, 2


def conv1d_stream_slots_forward(desc, x, hist_in, hist_out, w_packed, bias=None, add1=None, add1_hist=(None, None),
                                delay1=0, add2=None, add2_hist=(None, None), delay2=0, slots=None, rate=1, delay=0,
                                out=None):
    """:func:`conv1d_stream_delayed_forward` with a position per item: ``slots`` is a device ``(batch, SLOT_INTS)`` int32
    table -- per item the frames that went before (0: fresh, its state inputs read as zeros), the frames left, and
    ``SLOT_PAUSED`` / ``SLOT_LEFT_KNOWN`` -- from which, with the launch's ``rate`` (output columns per frame) and output
    ``delay``, the kernel derives each item's valid window.  A paused item's state is copied through and its output
    columns are zeros.  Every state input must be given.  One launch."""
    _require_device(w_packed)
    return _conv1d_stream_delayed(_lib.lib().pwg_conv1d_stream_slots_forward, "conv1d_stream_slots_forward", desc, x,
                                  hist_in, hist_out, w_packed, bias, add1, add1_hist, delay1, add2, add2_hist, delay2, None,
                                  out, (slots, rate, delay))


def conv1d_stream_slots_forward_bf16(desc, x, hist_in, hist_out, w_packed_bf16, bias=None, add1=None,
                                     add1_hist=(None, None), delay1=0, add2=None, add2_hist=(None, None), delay2=0,
                                     slots=None, rate=1, delay=0, out=None):
    """:func:`conv1d_stream_slots_forward` with bf16 operands, as :func:`conv1d_stream_delayed_forward_bf16` is to
    :func:`conv1d_stream_delayed_forward`."""
    _check_stream_image_bf16("conv1d_stream_slots_forward_bf16", desc, w_packed_bf16)
    return _conv1d_stream_delayed(_lib.lib().pwg_conv1d_stream_slots_forward_bf16, "conv1d_stream_slots_forward_bf16", desc,
                                  x, hist_in, hist_out, w_packed_bf16, bias, add1, add1_hist, delay1, add2, add2_hist,
                                  delay2, None, out, (slots, rate, delay))


def conv1d_stream_mirrored_supported(desc):
    """Does the mirrored form of the streaming kernel -- the reflect-padded layer of a non-causal network in a
    look-ahead stream -- cover this descriptor (the layer's causal descriptor with ``pad_mode="reflect"``)?  Host logic
    only; ``_lib.lib().pwg_last_error()`` names the reason for a False."""
    return bool(_lib.lib().pwg_conv1d_stream_mirrored_supported(ctypes.byref(desc)))


_I32_MAX = 2 ** 31 - 1


def conv1d_stream_mirrored_forward(desc, x, hist_in, hist_out, w_packed, bias=None, in_window=(0, None), valid=None,
                                   out=None):
    """:func:`conv1d_stream_delayed_forward` for a reflect-padded layer, without addends: the input is valid on
    ``in_window = (lo, hi)`` (chunk-relative input columns, unclamped: ``lo < 0`` lies in the history, ``hi`` None is not
    known yet) and a window column outside it reads its mirror image; history and chunk stay raw.  Output columns outside
    ``valid`` are stored as exact zeros.  One launch."""
    _require_device(x, hist_in, hist_out, w_packed, bias, out)
    out = _conv1d_stream_out(desc, x, hist_in, hist_out, None, None, out)
    lo, hi = (0, desc.t_out) if valid is None else valid
    in_lo, in_hi = in_window
    clamp = lambda v: max(-_I32_MAX, min(_I32_MAX, int(v)))  # noqa: E731  (the library saturates further)
    _lib.check(_lib.lib().pwg_conv1d_stream_mirrored_forward(
        ctypes.byref(desc), _ptr(x), _ptr(hist_in), _ptr(hist_out), _ptr(w_packed), _ptr(bias), _ptr(out), clamp(in_lo),
        _I32_MAX if in_hi is None else clamp(in_hi), int(lo), int(hi), _stream()), "conv1d_stream_mirrored_forward")
    return out


def conv1d_stream_slots_mirrored_forward(desc, x, hist_in, hist_out, w_packed, bias=None, slots=None, rate=1, delay=0,
                                         out=None):
    """:func:`conv1d_stream_mirrored_forward` with a position per item (utils.MelGANStreamPool):
    ``slots`` is the device table of :func:`conv1d_stream_slots_forward`, ``rate`` the launch's output columns per frame
    and ``delay`` its OUTPUT delay; the kernel derives each item's input window
    (``utils.streaming.slot_mirror_window``) and valid window itself.  A running item is the mirrored launch of that item
    alone with those windows, a fresh item reads ``hist_in`` as zeros, a paused item's history is copied through and its
    output columns are zeros.  ``hist_in`` must be given where the layer has history.  Coverage:
    :func:`conv1d_stream_mirrored_supported`.  One launch."""
    _require_device(x, hist_in, hist_out, w_packed, bias, out)
    out = _conv1d_stream_out(desc, x, hist_in, hist_out, None, None, out)
    if slots is not None:
        _slot_table("conv1d_stream_slots_mirrored_forward", slots, desc.batch)
    _lib.check(_lib.lib().pwg_conv1d_stream_slots_mirrored_forward(
        ctypes.byref(desc), _ptr(x), _ptr(hist_in), _ptr(hist_out), _ptr(w_packed), _ptr(bias), _ptr(slots), int(rate),
        int(delay), _ptr(out), _stream()), "conv1d_stream_slots_mirrored_forward")
    return out


def pqmf_up_stream_slots(y, hist_in, hist_out, g, slots, pad):
    """``pwg_pqmf_up_stream`` with a position per item (``PQMF.stream_synthesis_slots``): ``y`` (B, K, n) sub-band
    columns, ``hist_in`` / ``hist_out`` (B, K, H), ``g`` (K, len) the synthesis taps, ``slots`` the device table of
    :func:`conv1d_stream_slots_forward` -> (B, K * n) samples, the chunk positions ``[-D, n - D)`` of every item.  A
    fresh item reads ``hist_in`` as zeros, a paused item's history is copied through and its samples are zeros.  One
    launch."""
    y = y.contiguous()
    _require_device(y, hist_in, hist_out, g)
    b, k, n = y.shape
    if slots is not None:
        _slot_table("pqmf_up_stream_slots", slots, b)
    assert g.is_contiguous() and g.dim() == 2 and g.shape[0] == k, (tuple(g.shape), k)
    for t in (hist_in, hist_out):
        assert t is None or (t.is_contiguous() and tuple(t.shape[:2]) == (b, k)), (tuple(t.shape), (b, k))
    x = torch.empty((b, k * n), device=y.device, dtype=torch.float32)
    _lib.check(_lib.lib().pwg_pqmf_up_stream_slots(_ptr(y), _ptr(hist_in), _ptr(hist_out), _ptr(g), _ptr(x), _ptr(slots), b,
                                                   n, k, g.shape[1], int(pad), _stream()), "pqmf_up_stream_slots")
    return x


def conv1d_stream_bf16_supported(desc):
    """Does the bf16-operand streaming kernel (csrc/conv1d_stream_bf16.hip) cover this descriptor?  It answers exactly
    as :func:`conv1d_stream_supported`.  Host logic only; ``_lib.lib().pwg_last_error()`` names the reason for a False."""
    return bool(_lib.lib().pwg_conv1d_stream_bf16_supported(ctypes.byref(desc)))


def _check_stream_image_bf16(name, desc, w_packed_bf16):
    """The image checks the two bf16 conv stream wrappers share."""
    if not w_packed_bf16.is_cuda or w_packed_bf16.dtype != torch.uint8:
        raise RuntimeError(f"{name}: w_packed_bf16 must be the device image of pack_weight_bf16")
    assert w_packed_bf16.numel() == _lib.lib().pwg_conv1d_bf16_packed_weight_bytes(ctypes.byref(_zero_padded(desc))), \
        f"{name}: w_packed_bf16 is not this layer's bf16 image"


def conv1d_stream_forward_bf16(desc, x, hist_in, hist_out, w_packed_bf16, bias=None, add1=None, add2=None, out=None):
    """:func:`conv1d_stream_forward` with bf16 operands: the activated window and the weights (``w_packed_bf16``, the
    image of :func:`pack_weight_bf16`) are bf16, accumulation / epilogue / tensors / history fp32; ``hist_out`` is
    bit-identical to the fp32 launch's."""
    _require_device(x, hist_in, hist_out, bias, add1, add2, out)
    _check_stream_image_bf16("conv1d_stream_forward_bf16", desc, w_packed_bf16)
    out = _conv1d_stream_out(desc, x, hist_in, hist_out, add1, add2, out)
    _lib.check(_lib.lib().pwg_conv1d_stream_bf16_forward(ctypes.byref(desc), _ptr(x), _ptr(hist_in), _ptr(hist_out),
                                                         _ptr(w_packed_bf16), _ptr(bias), _ptr(add1), _ptr(add2),
                                                         _ptr(out), _stream()), "conv1d_stream_bf16_forward")
    return out


def conv1d_stream_bf16_delayed_supported(desc, delay1=0, delay2=0):
    """Does the delayed form of the bf16-operand streaming kernel cover this descriptor and these addend delays?  It
    answers exactly as :func:`conv1d_stream_delayed_supported`, with the same ``pwg_last_error`` reason.  Host logic
    only."""
    return bool(_lib.lib().pwg_conv1d_stream_bf16_delayed_supported(ctypes.byref(desc), int(delay1), int(delay2)))


def conv1d_stream_delayed_forward_bf16(desc, x, hist_in, hist_out, w_packed_bf16, bias=None, add1=None,
                                       add1_hist=(None, None), delay1=0, add2=None, add2_hist=(None, None), delay2=0,
                                       valid=None, out=None):
    """:func:`conv1d_stream_delayed_forward` with bf16 operands (``w_packed_bf16``: the image of
    :func:`pack_weight_bf16`), as :func:`conv1d_stream_forward_bf16` is to :func:`conv1d_stream_forward`: accumulation,
    epilogue, addends, tensors, history and delay lines are fp32, and the state written is bit-identical to the fp32
    delayed launch's.  One launch."""
    _check_stream_image_bf16("conv1d_stream_delayed_forward_bf16", desc, w_packed_bf16)
    return _conv1d_stream_delayed(_lib.lib().pwg_conv1d_stream_bf16_delayed_forward, "conv1d_stream_bf16_delayed_forward",
                                  desc, x, hist_in, hist_out, w_packed_bf16, bias, add1, add1_hist, delay1, add2,
                                  add2_hist, delay2, valid, out)


def make_resunit_desc(batch, channels, t, kernel, dilation, has_conv2=True, slope1=0.1, slope2=0.1, out_div=1.0):
    return ResUnitDesc(int(batch), int(channels), int(t), int(kernel), int(dilation), int(bool(has_conv2)),
                       float(slope1), float(slope2), float(out_div))


def resunit_supported(desc):
    """Does the one-launch residual unit (csrc/resunit.hip) cover this geometry?"""
    return bool(_lib.lib().pwg_resunit_supported(ctypes.byref(desc)))


def resunit_profitable(desc):
    """Supported AND measured faster than the separate convolutions (heuristic lives with the kernel)."""
    return bool(_lib.lib().pwg_resunit_profitable(ctypes.byref(desc)))


def resunit_pack_weight(w, scale=None):
    """torch-layout (C, C, k) weight (+ optional weight-norm row scale) -> MFMA A-operand image."""
    _require_device(w, scale)
    c, k = w.shape[0], w.shape[2]
    assert w.shape[1] == c
    out = torch.empty(_lib.lib().pwg_resunit_packed_weight_floats(c, k), device=w.device, dtype=torch.float32)
    _lib.check(_lib.lib().pwg_resunit_pack_weight(c, k, _ptr(w), _ptr(scale), _ptr(out), _stream()),
               "resunit_pack_weight")
    return out


def resunit_forward(desc, x, w1_packed, b1, w2_packed=None, b2=None, add2=None, out=None):
    """One MRF residual unit: ``(x + conv2(lrelu(conv1(lrelu(x)) + b1)) + b2 [+ add2]) [/ out_div]``."""
    _require_device(x, w1_packed, b1, w2_packed, b2, add2, out)
    assert x.numel() == desc.batch * desc.channels * desc.t
    if out is None:
        out = torch.empty_like(x)
    _lib.check(_lib.lib().pwg_resunit_forward(ctypes.byref(desc), _ptr(x), _ptr(w1_packed), _ptr(b1), _ptr(w2_packed),
                                              _ptr(b2), _ptr(add2), _ptr(out), _stream()), "resunit_forward")
    return out


def resunit_split_supported(desc):
    """Does the split-operand residual unit (csrc/resunit_split.hip) cover this geometry?  Host logic only (no device
    needed); ``_lib.lib().pwg_last_error()`` names the reason for a False."""
    return bool(_lib.lib().pwg_resunit_split_supported(ctypes.byref(desc)))


def resunit_forward_split(desc, x, w1_split, b1, w2_split=None, b2=None, add2=None, out=None, mfma_shape=None):
    """:func:`resunit_forward` computed on the bf16 MFMA from 3-way split operands (inference only).
    ``w1_split`` / ``w2_split``: the images of :func:`pack_weight_split` for the unit's convolutions; ``mfma_shape``
    (tuning / tests): 32 or 16 selects the MFMA instruction."""
    _require_device(x, b1, b2, add2, out)
    for w in (w1_split, w2_split):
        if w is not None and (not w.is_cuda or w.dtype != torch.uint8):
            raise RuntimeError("resunit_forward_split: the weights must be device images of pack_weight_split")
    assert x.numel() == desc.batch * desc.channels * desc.t
    image_bytes = 6 * desc.kernel * desc.channels * desc.channels  # three bf16 parts of a (C, C, k) weight
    for w in (w1_split, w2_split):
        assert w is None or w.numel() == image_bytes, "resunit_forward_split: not this unit's split image"
    assert add2 is None or add2.numel() == x.numel()
    if out is None:
        out = torch.empty_like(x)
    args = (ctypes.byref(desc), _ptr(x), _ptr(w1_split), _ptr(b1), _ptr(w2_split), _ptr(b2), _ptr(add2), _ptr(out))
    if mfma_shape is None:
        rc = _lib.lib().pwg_resunit_split_forward(*args, _stream())
    else:
        rc = _lib.lib().pwg_resunit_split_forward_cfg(*args, int(mfma_shape), _stream())
    _lib.check(rc, "resunit_split_forward")
    return out


def resblock_split_supported(desc, dilations):
    """Does the chained block of split-operand units (``resblock_split_kernel``, csrc/resunit_split.hip) cover
    ``len(dilations)`` pair-form units of this geometry?  Host logic only; ``_lib.lib().pwg_last_error()`` names the
    reason for a False.  ``desc.dilation`` and the descriptor's slopes are not read."""
    dil = (ctypes.c_int32 * len(dilations))(*[int(v) for v in dilations])
    return bool(_lib.lib().pwg_resblock_split_supported(ctypes.byref(desc), len(dilations), dil))


def resblock_split_frame(desc, dilations):
    """The frame of the chained block: dict of ``H`` (columns every phase computes), ``bn_out`` (columns a frame
    stores), ``edge`` (frame columns in front of the first stored one: a frame starts at ``t0 - edge``), ``margin``,
    ``lds`` and ``tiles``.  Host logic only."""
    dil = (ctypes.c_int32 * len(dilations))(*[int(v) for v in dilations])
    out = (ctypes.c_int32 * 6)()
    _lib.check(_lib.lib().pwg_resblock_split_frame(ctypes.byref(desc), len(dilations), dil, out), "resblock_split_frame")
    return dict(zip(("H", "bn_out", "edge", "margin", "lds", "tiles"), (int(v) for v in out)))


def resblock_forward_split(desc, x, dilations, slopes1, slopes2, w1_split, b1, w2_split, b2, add2=None, out=None,
                           mfma_shape=None):
    """``len(dilations)`` chained :func:`resunit_forward_split` units (pair form) as ONE launch, bit for bit the chain
    at the same MFMA shape: the last unit takes ``add2`` and ``desc.out_div`` (inference only).
    ``w1_split`` / ``b1`` / ``w2_split`` / ``b2``: one entry per unit (a bias may be None)."""
    n = len(dilations)
    assert len(slopes1) == len(slopes2) == len(w1_split) == len(b1) == len(w2_split) == len(b2) == n
    _require_device(x, add2, out, *b1, *b2)
    image_bytes = 6 * desc.kernel * desc.channels * desc.channels  # three bf16 parts of a (C, C, k) weight
    for w in (*w1_split, *w2_split):
        if w is None or not w.is_cuda or w.dtype != torch.uint8:
            raise RuntimeError("resblock_forward_split: the weights must be device images of pack_weight_split")
        assert w.numel() == image_bytes, "resblock_forward_split: not this unit's split image"
    assert x.numel() == desc.batch * desc.channels * desc.t
    assert add2 is None or add2.numel() == x.numel()
    if out is None:
        out = torch.empty_like(x)

    def ptrs(ts):
        return (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])

    _lib.check(_lib.lib().pwg_resblock_split_forward_cfg(
        ctypes.byref(desc), n, (ctypes.c_int32 * n)(*[int(v) for v in dilations]),
        (ctypes.c_float * n)(*[float(v) for v in slopes1]), (ctypes.c_float * n)(*[float(v) for v in slopes2]), _ptr(x),
        ptrs(w1_split), ptrs(b1), ptrs(w2_split), ptrs(b2), _ptr(add2), _ptr(out),
        16 if mfma_shape is None else int(mfma_shape), _stream()), "resblock_split_forward")
    return out


def _require_frames(frames, batch, what):
    """The device table of a ragged batch: int32 ``(batch,)``, contiguous."""
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
        raise RuntimeError(f"{what}: the frames table must be a device tensor; there is no CPU fallback path")
    if frames.dtype != torch.int32 or tuple(frames.shape) != (int(batch),) or not frames.is_contiguous():
        raise RuntimeError(f"{what}: the frames table must be a contiguous int32 tensor of shape ({int(batch)},), got "
                           f"{frames.dtype} {tuple(frames.shape)}")


def zero_tail(y, frames, rate):
    """Stores exact zeros at the columns ``>= frames[b] * rate`` of every row of item ``b`` of ``y`` (B, C, T), in place
    (csrc/elementwise.hip; write-only: the tail may hold anything before).  ``frames``: device int32 ``(B,)``; ``rate``:
    columns of ``y`` per frame.  Behind any convolution launch it re-establishes the invariant of a ragged forward
    (DESIGN.md s9.4).  Returns ``y``."""
    _require_device(y)
    if y.dim() != 3:
        raise RuntimeError(f"zero_tail: expected a (B, C, T) tensor, got {tuple(y.shape)}")
    _require_frames(frames, y.shape[0], "zero_tail")
    _lib.check(_lib.lib().pwg_zero_tail(_ptr(y), _ptr(frames), y.shape[0], y.shape[1], y.shape[2], int(rate), _stream()),
               "zero_tail")
    return y


def mirror_tail(y, frames, rate, pad):
    """:func:`zero_tail` with the mirror a reflect-padded consumer reads (csrc/elementwise.hip), in place:
    with ``e = frames[b] * rate`` the columns ``e + j``, ``0 <= j < pad``, of item ``b`` receive ``y[b, :, e - 2 - j]``
    (``ReflectionPad1d``'s image of the item's own last columns) and every column ``>= e + pad`` an exact zero.
    ``pad = 0`` is :func:`zero_tail`; an item of 0 frames becomes all zeros; an item not longer than ``pad`` gets
    unspecified mirror values (reflection is undefined for it).  Returns ``y``."""
    _require_device(y)
    if y.dim() != 3:
        raise RuntimeError(f"mirror_tail: expected a (B, C, T) tensor, got {tuple(y.shape)}")
    _require_frames(frames, y.shape[0], "mirror_tail")
    _lib.check(_lib.lib().pwg_mirror_tail(_ptr(y), _ptr(frames), y.shape[0], y.shape[1], y.shape[2], int(rate), int(pad),
                                          _stream()), "mirror_tail")
    return y


def _ragged_3d(what, frames, *tensors):
    """The checks the ragged TADE wrappers share: contiguous fp32 device (B, C, T) tensors and the table."""
    _require_device(*tensors)
    for t in tensors:
        if t is not None and t.dim() != 3:
            raise RuntimeError(f"{what}: expected a (B, C, T) tensor, got {tuple(t.shape)}")
    _require_frames(frames, tensors[0].shape[0], what)


def instance_norm_ragged(x, frames, rate, eps=1e-5):
    """``InstanceNorm1d(affine=False)`` over a ragged batch (csrc/tade_ragged.hip): the statistics of item
    ``b`` of ``x`` (B, C, T) run over its columns ``[0, e)``, ``e = min(frames[b] * rate, T)``; below ``e`` the result is
    bit for bit the plain kernel on the item alone, at and past ``e`` it is ``+0.0`` (nothing there is read).  Forward
    only."""
    _ragged_3d("instance_norm_ragged", frames, x)
    y = torch.empty_like(x)
    b, c, t = x.shape
    _lib.check(_lib.lib().pwg_instance_norm_ragged(_ptr(x), _ptr(y), _ptr(frames), b, c, t, int(rate), float(eps),
                                                   _stream()), "instance_norm_ragged")
    return y


def upsample_nearest_ragged(x, scale, frames, rate_out, add=None):
    """``nearest_upsample(x, scale) (+ add)`` over a ragged batch: x (B, C, T) -> (B, C, T * scale) whose item ``b``
    ends at ``e = min(frames[b] * rate_out, T * scale)`` (``rate_out``: OUTPUT columns per frame); zeros from ``e`` on,
    nothing of ``x`` or ``add`` read there."""
    _ragged_3d("upsample_nearest_ragged", frames, x, add)
    b, c, t = x.shape
    y = torch.empty((b, c, t * int(scale)), device=x.device, dtype=torch.float32)
    if add is not None and add.shape != y.shape:
        raise RuntimeError(f"upsample_nearest_ragged: add must be {tuple(y.shape)}, got {tuple(add.shape)}")
    _lib.check(_lib.lib().pwg_upsample_nearest_ragged(_ptr(x), _ptr(add), _ptr(y), _ptr(frames), b, c, t, int(scale),
                                                      int(rate_out), _stream()), "upsample_nearest_ragged")
    return y


def tade_modulate_ragged(xn, cg, scale, frames, rate_out):
    """``cg[:, :C] * nearest_upsample(xn, scale) + cg[:, C:]`` over a ragged batch: xn (B, C, T), cg (B, 2C, T * scale) ->
    (B, C, T * scale), item ``b`` ending at ``min(frames[b] * rate_out, T * scale)``; zeros from there on."""
    _ragged_3d("tade_modulate_ragged", frames, xn, cg)
    b, c, t = xn.shape
    if tuple(cg.shape) != (b, 2 * c, t * int(scale)):
        raise RuntimeError(f"tade_modulate_ragged: cg must be {(b, 2 * c, t * int(scale))}, got {tuple(cg.shape)}")
    y = torch.empty((b, c, t * int(scale)), device=xn.device, dtype=torch.float32)
    _lib.check(_lib.lib().pwg_tade_modulate_ragged(_ptr(xn), _ptr(cg), _ptr(y), _ptr(frames), b, c, t, int(scale),
                                                   int(rate_out), _stream()), "tade_modulate_ragged")
    return y


def softmax_gate_ragged(z, use_softmax, frames, rate):
    """The gate of ``TADEResBlock`` over a ragged batch: z (B, 2C, T) -> (B, C, T), softmax over channels (or sigmoid) of
    the first half x tanh of the second below ``min(frames[b] * rate, T)``, zeros from there on."""
    _ragged_3d("softmax_gate_ragged", frames, z)
    b, c2, t = z.shape
    if c2 % 2:
        raise RuntimeError(f"softmax_gate_ragged: expected an even number of channels, got {c2}")
    y = torch.empty((b, c2 // 2, t), device=z.device, dtype=torch.float32)
    _lib.check(_lib.lib().pwg_softmax_gate_ragged(_ptr(z), _ptr(y), _ptr(frames), b, c2 // 2, t, int(rate),
                                                  int(bool(use_softmax)), _stream()), "softmax_gate_ragged")
    return y


def resunit_split_ragged_supported(desc, rate):
    """Does the ragged form of the split-operand residual unit cover this geometry at ``rate`` columns per frame?
    :func:`resunit_split_supported` plus ``rate % 4 == 0``.  Host logic only; ``_lib.lib().pwg_last_error()`` names the
    reason for a False."""
    return bool(_lib.lib().pwg_resunit_split_ragged_supported(ctypes.byref(desc), int(rate)))


def resunit_forward_split_ragged(desc, x, frames, rate, w1_split, b1, w2_split=None, b2=None, add2=None, out=None,
                                 mfma_shape=16):
    """:func:`resunit_forward_split` over a ragged batch: item ``b`` ends at column ``min(frames[b] * rate, T)``.  ``x``
    and ``add2`` must be zero past their items' ends (:func:`zero_tail`); the output is, per item, bit for bit the plain
    unit on the item alone up to its end and exact zeros past it.  ``mfma_shape``: as there (16: the default shape)."""
    _require_device(x, b1, b2, add2, out)
    for w in (w1_split, w2_split):
        if w is not None and (not w.is_cuda or w.dtype != torch.uint8):
            raise RuntimeError("resunit_forward_split_ragged: the weights must be device images of pack_weight_split")
    _require_frames(frames, desc.batch, "resunit_forward_split_ragged")
    assert x.numel() == desc.batch * desc.channels * desc.t
    image_bytes = 6 * desc.kernel * desc.channels * desc.channels  # three bf16 parts of a (C, C, k) weight
    for w in (w1_split, w2_split):
        assert w is None or w.numel() == image_bytes, "resunit_forward_split_ragged: not this unit's split image"
    assert add2 is None or add2.numel() == x.numel()
    if out is None:
        out = torch.empty_like(x)
    _lib.check(_lib.lib().pwg_resunit_split_forward_ragged(
        ctypes.byref(desc), _ptr(x), _ptr(w1_split), _ptr(b1), _ptr(w2_split), _ptr(b2), _ptr(add2), _ptr(out),
        int(mfma_shape), _ptr(frames), int(rate), _stream()), "resunit_split_forward_ragged")
    return out


def resstack_supported(channels, t, dilation):
    """Does the one-launch MelGAN residual stack (csrc/resstack.hip) cover this geometry?"""
    return bool(_lib.lib().pwg_resstack_supported(int(channels), int(t), int(dilation)))


def resstack_pack_weight(w1, s1, w2, s2, ws, ss):
    """(C, C, 3), (C, C, 1), (C, C, 1) weights (+ optional weight-norm row scales) -> the unit's MFMA A-operand image."""
    _require_device(w1, s1, w2, s2, ws, ss)
    c = w1.shape[0]
    n = _lib.lib().pwg_resstack_packed_weight_floats(c)
    if n == 0:
        _lib.check(-1, "resstack_packed_weight_floats")
    out = torch.empty(n, device=w1.device, dtype=torch.float32)
    _lib.check(_lib.lib().pwg_resstack_pack_weight(c, _ptr(w1), _ptr(s1), _ptr(w2), _ptr(s2), _ptr(ws), _ptr(ss), _ptr(out),
                                                   _stream()), "resstack_pack_weight")
    return out


def resstack_forward(x, w_packed, dilation, slope, b1=None, b2=None, bs=None, save_h=False):
    """y (and h, the dilated convolution's pre-activation output, when ``save_h``) of one residual stack."""
    _require_device(x, w_packed, b1, b2, bs)
    b, c, t = x.shape
    y = torch.empty_like(x)
    h = torch.empty_like(x) if save_h else None
    _lib.check(_lib.lib().pwg_resstack_forward(b, c, t, int(dilation), float(slope), _ptr(x), _ptr(w_packed), _ptr(b1), _ptr(b2),
                                               _ptr(bs), _ptr(y), _ptr(h), _stream()), "resstack_forward")
    return y, h


def resstack_ragged_supported(channels, t, dilation, rate):
    """Does the ragged form of the one-launch residual stack cover this geometry at ``rate`` columns per frame?
    :func:`resstack_supported` plus ``rate >= 4`` and ``rate % 4 == 0``.  Host logic only."""
    return bool(_lib.lib().pwg_resstack_ragged_supported(int(channels), int(t), int(dilation), int(rate)))


def resstack_forward_ragged(x, frames, rate, w_packed, dilation, slope, b1=None, b2=None, bs=None, out=None):
    """:func:`resstack_forward` over a ragged batch (inference: no ``h``): item ``b`` is the sequence ``[0, frames[b] *
    rate)`` of its rows, the reflection mirrors at its end, ``x`` may hold anything past it, and ``y`` holds exact zeros
    there.  Per item bit for bit the plain unit on the item alone."""
    _require_device(x, w_packed, b1, b2, bs, out)
    if x.dim() != 3 or not x.is_contiguous():
        raise RuntimeError(f"resstack_forward_ragged: expected a contiguous (B, C, T) tensor, got {tuple(x.shape)}")
    b, c, t = x.shape
    _require_frames(frames, b, "resstack_forward_ragged")
    if out is None:
        out = torch.empty_like(x)
    assert out.shape == x.shape and out.is_contiguous()
    _lib.check(_lib.lib().pwg_resstack_forward_ragged(b, c, t, int(dilation), float(slope), _ptr(x), _ptr(w_packed),
                                                      _ptr(b1), _ptr(b2), _ptr(bs), _ptr(out), _ptr(frames), int(rate),
                                                      _stream()), "resstack_forward_ragged")
    return out


def resstack_pack_weight_bwd(w1, s1, w2, s2, ws, ss):
    """The unit's weights re-laid for its data gradient (transposed; weight-norm scales on the reduction index)."""
    _require_device(w1, s1, w2, s2, ws, ss)
    c = w1.shape[0]
    n = _lib.lib().pwg_resstack_packed_weight_floats(c)
    if n == 0:
        _lib.check(-1, "resstack_packed_weight_floats")
    out = torch.empty(n, device=w1.device, dtype=torch.float32)
    _lib.check(_lib.lib().pwg_resstack_pack_weight_bwd(c, _ptr(w1), _ptr(s1), _ptr(w2), _ptr(s2), _ptr(ws), _ptr(ss),
                                                       _ptr(out), _stream()), "resstack_pack_weight_bwd")
    return out


def resstack_backward_data(dy, h, x, w_packed_bwd, dilation, slope):
    """(dh, dxp): gradient w.r.t. the dilated convolution's output and w.r.t. its reflect-padded input (+ the skip
    branch's contribution at the interior positions), shapes (B, C, T) and (B, C, T + 2 * dilation)."""
    _require_device(dy, h, x, w_packed_bwd)
    b, c, t = x.shape
    dh = torch.empty_like(x)
    dxp = torch.empty((b, c, t + 2 * int(dilation)), device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().pwg_resstack_backward_data(b, c, t, int(dilation), float(slope), _ptr(dy), _ptr(h), _ptr(x),
                                                     _ptr(w_packed_bwd), _ptr(dh), _ptr(dxp), _stream()),
               "resstack_backward_data")
    return dh, dxp


def make_wavenet_desc(batch, t, dilation, residual_channels=64, gate_channels=128, skip_channels=64, aux_channels=80,
                      kernel=3, causal=False, out_mul=1.0, skip_mul=1.0):
    return WaveNetDesc(int(batch), int(t), int(residual_channels), int(gate_channels), int(skip_channels),
                       int(aux_channels), int(kernel), int(dilation), int(bool(causal)), float(out_mul), float(skip_mul))


def wavenet_layer_supported(desc):
    """Does the one-launch WaveNet layer (csrc/wavenet.hip) cover this geometry?"""
    return bool(_lib.lib().pwg_wavenet_layer_supported(ctypes.byref(desc)))


def wavenet_pack_weights(desc, w_dil, s_dil, w_aux, s_aux, w_skip, s_skip, w_out, s_out):
    """The four torch-layout weights of a layer (+ optional weight-norm row scales) -> one MFMA A-operand image."""
    _require_device(w_dil, s_dil, w_aux, s_aux, w_skip, s_skip, w_out, s_out)
    out = torch.empty(_lib.lib().pwg_wavenet_packed_weight_floats(ctypes.byref(desc)), device=w_dil.device,
                      dtype=torch.float32)
    _lib.check(_lib.lib().pwg_wavenet_pack_weights(ctypes.byref(desc), _ptr(w_dil), _ptr(s_dil), _ptr(w_aux), _ptr(s_aux),
                                                   _ptr(w_skip), _ptr(s_skip), _ptr(w_out), _ptr(s_out), _ptr(out),
                                                   _stream()), "wavenet_pack_weights")
    return out


def wavenet_layer_forward(desc, x, c, skips, packed, b_dil, b_skip, b_out, save=False, skips_out=None):
    """One gated residual layer in one launch -> (x_out, skips_out, z, g); ``z`` / ``g`` only with ``save``
    (training: the backward pass needs them).  ``skips_out`` may be ``skips`` itself (in-place running sum)."""
    _require_device(x, c, skips, packed, b_dil, b_skip, b_out, skips_out)
    x_out = torch.empty_like(x)
    if skips_out is None:
        skips_out = torch.empty_like(x)
    z = torch.empty((x.shape[0], desc.gate_channels, x.shape[2]), device=x.device, dtype=torch.float32) if save else None
    g = torch.empty_like(x) if save else None
    _lib.check(_lib.lib().pwg_wavenet_layer_forward(ctypes.byref(desc), _ptr(x), _ptr(c), _ptr(skips), _ptr(packed),
                                                    _ptr(b_dil), _ptr(b_skip), _ptr(b_out), _ptr(x_out), _ptr(skips_out),
                                                    _ptr(z), _ptr(g), _stream()), "wavenet_layer_forward")
    return x_out, skips_out, z, g


def wavenet_stream_supported(desc):
    """Does the streaming form of the causal layer (csrc/wavenet_stream.hip) cover this geometry, ``desc.t`` = columns
    per push?  Host logic only (no device needed); ``_lib.lib().pwg_last_error()`` names the reason for a False."""
    return bool(_lib.lib().pwg_wavenet_stream_supported(ctypes.byref(desc)))


def wavenet_stream_hist_floats(desc):
    """Floats of one history buffer of the layer: ``batch * 64 * (kernel - 1) * dilation`` (0: unsupported)."""
    return _lib.lib().pwg_wavenet_stream_hist_floats(ctypes.byref(desc))


def _wavenet_stream(entry, name, desc, x, c, skips, hist_in, hist_out, packed, b_dil, b_skip, b_out, bf16=False,
                    delayed=None, valid=None, slots=None, skips_out=None, save=None):
    """What the gated layer's stream wrappers share: the checks of every tensor and the call of the library's ``entry``.
    ``bf16``: ``packed`` is the image of :func:`wavenet_bf16_pack_weights`; ``delayed``: None for the causal form, else
    ``(c_line, c_delay, skip_line)`` of a delayed or slotted one, which takes its position behind the biases -- the window
    ``valid``, or ``slots = (table, rate, delay)``; ``save``: None for an entry without the ``z`` / ``g`` outputs, else
    whether to allocate and return them."""
    c_line, c_delay, skip_line = (None, 0, (None, None)) if delayed is None else delayed
    line_in, line_out = skip_line if skips is not None else (None, None)
    _require_device(x, c, c_line, skips, line_in, line_out, hist_in, hist_out, *(() if bf16 else (packed,)), b_dil, b_skip,
                    b_out, skips_out)
    if bf16:
        _bf16_stream_image(name, packed)
    if slots is not None:
        _slot_table(name, slots[0], desc.batch)
    assert x.numel() == desc.batch * desc.residual_channels * desc.t, (tuple(x.shape), desc.batch, desc.t)
    assert c.numel() == desc.batch * desc.aux_channels * desc.t, (tuple(c.shape), desc.batch, desc.t)
    n_hist = (wavenet_stream_hist_floats if delayed is None else wavenet_stream_delayed_hist_floats)(desc)
    for t in (hist_in, hist_out):
        assert t is None or n_hist == 0 or t.numel() == n_hist, (tuple(t.shape), n_hist)
    x_out = torch.empty_like(x)
    if skips_out is None:
        skips_out = torch.empty_like(x)
    for t in (skips, skips_out):
        assert t is None or t.numel() == x.numel()
    cond = lines = position = ()
    if delayed is not None:
        for t in (line_in, line_out):
            assert t is None or t.numel() == desc.batch * desc.skip_channels * desc.dilation, tuple(t.shape)
        c_cols = 0
        if c_line is not None:
            assert c_line.is_contiguous() and c_line.numel() % (desc.batch * desc.aux_channels) == 0, tuple(c_line.shape)
            c_cols = c_line.numel() // (desc.batch * desc.aux_channels)
        cond, lines = (_ptr(c_line), c_cols, int(c_delay)), (_ptr(line_in), _ptr(line_out))
        if slots is None:
            lo, hi = (0, desc.t) if valid is None else valid
            position = (int(lo), int(hi))
        else:
            position = (_ptr(slots[0]), int(slots[1]), int(slots[2]))
    z = torch.empty((x.shape[0], desc.gate_channels, x.shape[2]), device=x.device, dtype=torch.float32) if save else None
    g = torch.empty_like(x) if save else None
    _lib.check(entry(ctypes.byref(desc), _ptr(x), _ptr(c), *cond, _ptr(skips), *lines, _ptr(hist_in), _ptr(hist_out),
                     _ptr(packed), _ptr(b_dil), _ptr(b_skip), _ptr(b_out), *position, _ptr(x_out), _ptr(skips_out),
                     *(() if save is None else (_ptr(z), _ptr(g))), _stream()), name)
    return (x_out, skips_out, z, g) if save else (x_out, skips_out)


def wavenet_stream_forward(desc, x, c, skips, hist_in, hist_out, packed, b_dil, b_skip, b_out, skips_out=None):
    """One chunk of a causal gated residual layer's stream in one launch -> (x_out, skips_out); also writes
    ``hist_out`` = the last H columns of ``concat(hist_in, x)``.  ``hist_in`` None: start of stream (zero left context).
    ``hist_in`` and ``hist_out`` must be distinct buffers; ``skips_out`` may be ``skips`` itself."""
    return _wavenet_stream(_lib.lib().pwg_wavenet_stream_forward, "wavenet_stream_forward", desc, x, c, skips, hist_in,
                           hist_out, packed, b_dil, b_skip, b_out, skips_out=skips_out)


def stretch_conv_stream(x, hist_in, hist_out, w, scale, freq_kernel=1, act=None, slope=0.0):
    """One chunk of a causal upsampler stage's stream (nearest stretch x ``scale`` + the 1 x (2 scale + 1) conv with
    left padding 2 scale) in one launch: x (B, C, n) -> (B, C, n * scale); ``hist_in`` / ``hist_out`` (B, C, 2): the
    last two raw input columns (``hist_in`` None: zeros), distinct buffers."""
    x = x.contiguous()
    w = w.reshape(-1).contiguous()
    _require_device(x, hist_in, hist_out, w)
    b, ch, n = x.shape
    assert w.numel() == (2 * scale + 1) * freq_kernel, (w.numel(), scale, freq_kernel)
    for t in (hist_in, hist_out):
        assert t is None or t.numel() == b * ch * 2, tuple(t.shape)
    y = torch.empty((b, ch, n * scale), device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().pwg_stretch_conv_stream(_ptr(x), _ptr(hist_in), _ptr(hist_out), _ptr(w), _ptr(y), b * ch, n,
                                                  int(scale), int(freq_kernel), ACT[act], float(slope), _stream()),
               "stretch_conv_stream")
    return y


def wavenet_stream_delayed_supported(desc, c_delay=0):
    """Does the delayed form of the streaming layer (csrc/wavenet_stream.hip; the NON-causal layer in a stream with a
    fixed look-ahead) cover this geometry with the conditioning read ``c_delay`` columns late?  ``desc`` is the layer's
    own (``causal == 0``).  Host logic only; ``_lib.lib().pwg_last_error()`` names the reason for a False."""
    return bool(_lib.lib().pwg_wavenet_stream_delayed_supported(ctypes.byref(desc), int(c_delay)))


def wavenet_stream_delayed_hist_floats(desc):
    """Floats of one history buffer of the layer in delayed form: ``batch * 64 * 2 * dilation`` (0: unsupported)."""
    return _lib.lib().pwg_wavenet_stream_delayed_hist_floats(ctypes.byref(desc))


def wavenet_stream_delayed_forward(desc, x, c, c_line, c_delay, skips, skip_line, hist_in, hist_out, packed, b_dil, b_skip,
                                   b_out, valid=None):
    """One chunk of a NON-causal gated residual layer streamed with a fixed look-ahead, in one launch -> (x_out,
    skips_out), both ``dilation`` columns later than ``x``.  The conditioning of output column ``j`` is column
    ``j - c_delay`` of ``concat(c_line, c)`` counted from the chunk (``c_line`` (B, 80, L), None: zeros); the skip addend
    is ``concat(skip_line[0], skips)[j]`` and ``skip_line[1]`` receives the last ``dilation`` columns of that
    concatenation (``skip_line = (line_in, line_out)``, each (B, 64, dilation); ignored without ``skips``); ``hist_out`` =
    the last ``2 * dilation`` columns of ``concat(hist_in, x)``.  Columns outside ``valid = (lo, hi)`` (None: all are
    valid) are stored as exact zeros in both outputs."""
    return _wavenet_stream(_lib.lib().pwg_wavenet_stream_delayed_forward, "wavenet_stream_delayed_forward", desc, x, c, skips,
                           hist_in, hist_out, packed, b_dil, b_skip, b_out, delayed=(c_line, c_delay, skip_line), valid=valid)


def stretch_conv_stream_delayed(x, hist_in, hist_out, w, scale, freq_kernel=1, act=None, slope=0.0, valid=None):
    """:func:`stretch_conv_stream` for the NON-causal stage streamed with a fixed look-ahead (the causal stage on a time
    axis shifted by ``scale``): output columns outside ``valid = (lo, hi)`` (None: all are valid) are stored as exact
    zeros.  One launch."""
    x = x.contiguous()
    w = w.reshape(-1).contiguous()
    _require_device(x, hist_in, hist_out, w)
    b, ch, n = x.shape
    assert w.numel() == (2 * scale + 1) * freq_kernel, (w.numel(), scale, freq_kernel)
    for t in (hist_in, hist_out):
        assert t is None or t.numel() == b * ch * 2, tuple(t.shape)
    y = torch.empty((b, ch, n * scale), device=x.device, dtype=torch.float32)
    lo, hi = (0, n * scale) if valid is None else valid
    _lib.check(_lib.lib().pwg_stretch_conv_stream_delayed(_ptr(x), _ptr(hist_in), _ptr(hist_out), _ptr(w), _ptr(y), b * ch, n,
                                                          int(scale), int(freq_kernel), ACT[act], float(slope), int(lo),
                                                          int(hi), _stream()), "stretch_conv_stream_delayed")
    return y


def delay_line_forward(x, line_in, line_out, delayed=False):
    """A delay line of a stream: ``line_out`` = the last L columns of ``concat(line_in, x)`` (x (B, C, n), lines
    (B, C, L), ``line_in`` None: zeros), also when ``n < L``.  ``delayed``: -> the first ``n`` columns of that
    concatenation (``x``, L columns late), else None.  One launch; copies only."""
    x = x.contiguous()
    _require_device(x, line_in, line_out)
    b, ch, n = x.shape
    L = line_out.shape[-1]
    for t in (line_in, line_out):
        assert t is None or (t.is_contiguous() and tuple(t.shape) == (b, ch, L)), (tuple(t.shape), (b, ch, L))
    out = torch.empty_like(x) if delayed else None
    _lib.check(_lib.lib().pwg_delay_line_forward(_ptr(x), _ptr(line_in), _ptr(line_out), _ptr(out), b * ch, n, L, _stream()),
               "delay_line_forward")
    return out


# ---- the slotted forms of the four launches above (utils.PWGStreamPool): one position per item, read
# from the device table of :func:`conv1d_stream_slots_forward`; every state input must be given

def _slot_table(name, slots, batch):
    if slots is None or not slots.is_cuda or slots.dtype != torch.int32 or not slots.is_contiguous():
        raise RuntimeError(f"{name}: slots must be a contiguous int32 device tensor (the kernel reads it; there is no CPU "
                           "fallback path)")
    assert tuple(slots.shape) == (batch, SLOT_INTS), (tuple(slots.shape), batch)
    return slots


def wavenet_stream_slots_forward(desc, x, c, c_line, c_delay, skips, skip_line, hist_in, hist_out, packed, b_dil, b_skip,
                                 b_out, slots=None, rate=1, delay=0, precision="fp32"):
    """:func:`wavenet_stream_delayed_forward` (``precision="bf16"``: :func:`wavenet_stream_delayed_forward_bf16`, on that
    image) with a position per item: the window gives way to ``slots``, the launch's ``rate`` (columns per frame) and
    output ``delay``.  A running item is the delayed launch with its own window, a fresh one reads ``hist_in``, ``c_line``
    and ``skip_line[0]`` as zeros, a paused one copies its state through and stores zeros.  One launch."""
    bf16 = precision == "bf16"
    name = "wavenet_stream_slots_forward_bf16" if bf16 else "wavenet_stream_slots_forward"
    return _wavenet_stream(getattr(_lib.lib(), "pwg_" + name), name, desc, x, c, skips, hist_in, hist_out, packed, b_dil,
                           b_skip, b_out, bf16=bf16, delayed=(c_line, c_delay, skip_line), slots=(slots, rate, delay))


def wavenet_stream_slots_forward_bf16(desc, x, c, c_line, c_delay, skips, skip_line, hist_in, hist_out, packed, b_dil,
                                      b_skip, b_out, slots=None, rate=1, delay=0):
    """:func:`wavenet_stream_slots_forward` with ``precision="bf16"``, named as the other bf16 wrappers are."""
    return wavenet_stream_slots_forward(desc, x, c, c_line, c_delay, skips, skip_line, hist_in, hist_out, packed, b_dil,
                                        b_skip, b_out, slots, rate, delay, precision="bf16")


def stretch_conv_stream_slots(x, hist_in, hist_out, w, scale, freq_kernel=1, act=None, slope=0.0, slots=None, rate=1,
                              delay=0):
    """:func:`stretch_conv_stream_delayed` with a position per item (item = the leading axis of ``x``): ``slots``, ``rate``
    (output columns per frame) and output ``delay`` stand where ``valid`` stood.  One launch."""
    x = x.contiguous()
    w = w.reshape(-1).contiguous()
    _require_device(x, hist_in, hist_out, w)
    b, ch, n = x.shape
    _slot_table("stretch_conv_stream_slots", slots, b)
    assert w.numel() == (2 * scale + 1) * freq_kernel, (w.numel(), scale, freq_kernel)
    for t in (hist_in, hist_out):
        assert t is None or (t.is_contiguous() and t.numel() == b * ch * 2), tuple(t.shape)
    y = torch.empty((b, ch, n * scale), device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().pwg_stretch_conv_stream_slots(_ptr(x), _ptr(hist_in), _ptr(hist_out), _ptr(w), _ptr(y), b, ch, n,
                                                        int(scale), int(freq_kernel), ACT[act], float(slope), _ptr(slots),
                                                        int(rate), int(delay), _stream()), "stretch_conv_stream_slots")
    return y


def delay_line_slots_forward(x, line_in, line_out, slots, delayed=False):
    """:func:`delay_line_forward` with a position per item (item = the leading axis of ``x``): a fresh item's line reads
    as zeros, a paused item's line is copied through and its delayed columns are zeros.  One launch; copies only."""
    x = x.contiguous()
    _require_device(x, line_in, line_out)
    b, ch, n = x.shape
    _slot_table("delay_line_slots_forward", slots, b)
    L = line_out.shape[-1]
    for t in (line_in, line_out):
        assert t is None or (t.is_contiguous() and tuple(t.shape) == (b, ch, L)), (tuple(t.shape), (b, ch, L))
    out = torch.empty_like(x) if delayed else None
    _lib.check(_lib.lib().pwg_delay_line_slots_forward(_ptr(x), _ptr(line_in), _ptr(line_out), _ptr(out), b, ch, n, L,
                                                       _ptr(slots), _stream()), "delay_line_slots_forward")
    return out


def slot_seed_history(x, hist, slots):
    """Writes column 0 of ``x`` (B, C, n) into every column of ``hist`` (B, C, H), in place, for the items whose row of
    ``slots`` says fresh and not paused; the other items' history is left as it is.  What ``conv_in`` of a Parallel
    WaveGAN pool starts an utterance from.  One launch."""
    x = x.contiguous()
    _require_device(x, hist)
    b, ch, n = x.shape
    _slot_table("slot_seed_history", slots, b)
    assert hist is None or (hist.is_contiguous() and tuple(hist.shape[:2]) == (b, ch)), tuple(hist.shape)
    cols = 1 if hist is None else hist.shape[-1]
    _lib.check(_lib.lib().pwg_slot_seed_history(_ptr(x), _ptr(hist), b, ch, n, cols, _ptr(slots), _stream()),
               "slot_seed_history")
    return hist


def wavenet_bf16_supported(desc):
    """Does the bf16-operand one-launch layer (csrc/wavenet_bf16.hip) cover this geometry?  Host logic only (no device
    needed); ``_lib.lib().pwg_last_error()`` names the reason for a False."""
    return bool(_lib.lib().pwg_wavenet_bf16_supported(ctypes.byref(desc)))


def wavenet_bf16_packed_weight_bytes(desc):
    n = _lib.lib().pwg_wavenet_bf16_packed_weight_bytes(ctypes.byref(desc))
    if n == 0:
        _lib.check(-1, "wavenet_bf16_packed_weight_bytes")
    return n


def wavenet_bf16_pack_weights(desc, w_dil, s_dil, w_aux, s_aux, w_skip, s_skip, w_out, s_out):
    """The four torch-layout fp32 weights of a layer (+ optional weight-norm row scales) -> one bf16 MFMA weight image
    (an opaque byte tensor); each effective weight ``w * scale`` is rounded to bf16 here, once."""
    _require_device(w_dil, s_dil, w_aux, s_aux, w_skip, s_skip, w_out, s_out)
    out = torch.empty(wavenet_bf16_packed_weight_bytes(desc), device=w_dil.device, dtype=torch.uint8)
    _lib.check(_lib.lib().pwg_wavenet_bf16_pack_weights(ctypes.byref(desc), _ptr(w_dil), _ptr(s_dil), _ptr(w_aux),
                                                        _ptr(s_aux), _ptr(w_skip), _ptr(s_skip), _ptr(w_out), _ptr(s_out),
                                                        _ptr(out), _stream()), "wavenet_bf16_pack_weights")
    return out


def wavenet_bf16_layer_forward(desc, x, c, skips, packed, b_dil, b_skip, b_out, save=False, skips_out=None,
                               mfma_shape=None):
    """One gated residual layer with bf16 operands (inference only) -> (x_out, skips_out, z, g); ``z`` (fp32) and ``g``
    (the bf16-rounded gate output, stored as fp32) only with ``save`` (stage tests).  ``skips_out`` may be ``skips``
    itself.  ``mfma_shape`` (tuning): 32 or 16 selects the MFMA instruction explicitly."""
    _require_device(x, c, skips, b_dil, b_skip, b_out, skips_out)
    if not packed.is_cuda or packed.dtype != torch.uint8:
        raise RuntimeError("wavenet_bf16_layer_forward: packed must be the device image of wavenet_bf16_pack_weights")
    assert tuple(x.shape) == (desc.batch, desc.residual_channels, desc.t) and x.is_contiguous(), tuple(x.shape)
    assert tuple(c.shape) == (desc.batch, desc.aux_channels, desc.t) and c.is_contiguous(), tuple(c.shape)
    for t in (skips, skips_out):
        assert t is None or (t.shape == x.shape and t.is_contiguous())
    x_out = torch.empty_like(x)
    if skips_out is None:
        skips_out = torch.empty_like(x)
    z = torch.empty((x.shape[0], desc.gate_channels, x.shape[2]), device=x.device, dtype=torch.float32) if save else None
    g = torch.empty_like(x) if save else None
    args = [ctypes.byref(desc), _ptr(x), _ptr(c), _ptr(skips), _ptr(packed), _ptr(b_dil), _ptr(b_skip), _ptr(b_out),
            _ptr(x_out), _ptr(skips_out), _ptr(z), _ptr(g)]
    if mfma_shape is None:
        rc = _lib.lib().pwg_wavenet_bf16_layer_forward(*args, _stream())
    else:
        rc = _lib.lib().pwg_wavenet_bf16_layer_forward_cfg(*args, int(mfma_shape), _stream())
    _lib.check(rc, "wavenet_bf16_layer_forward")
    return x_out, skips_out, z, g


def wavenet_layer_ragged_supported(desc, rate):
    """Do the ragged forms of the one-launch layer (fp32 and bf16) cover this geometry at ``rate`` columns per frame?
    :func:`wavenet_layer_supported` plus ``rate >= 4``, ``rate % 4 == 0``.  Host logic only (no device needed);
    ``_lib.lib().pwg_last_error()`` names the reason for a False."""
    return bool(_lib.lib().pwg_wavenet_layer_ragged_supported(ctypes.byref(desc), int(rate)))


def wavenet_layer_forward_ragged(desc, x, c, skips, frames, rate, packed, b_dil, b_skip, b_out, skips_out=None, x_out=None,
                                 bf16=False, mfma_shape=None):
    """One gated residual layer over a ragged batch in one launch (inference) -> (x_out, skips_out).
    Item ``b`` ends at column ``e = min(frames[b] * rate, T)``: ``x``, ``c`` and ``skips`` may hold anything at the
    columns ``>= e`` (they read as zero), the outputs are NOT written there (fresh outputs are ``torch.empty``), and the
    columns ``< e`` are bit for bit the plain layer's on the item alone.  ``skips_out`` may be ``skips`` itself.
    ``bf16``: the bf16-operand layer on the image of :func:`wavenet_bf16_pack_weights` (``mfma_shape``: 32 or 16, None =
    the default), else the fp32 layer on the image of :func:`wavenet_pack_weights`."""
    _require_device(x, c, skips, b_dil, b_skip, b_out, skips_out, x_out)
    what = "wavenet_layer_forward_ragged"
    if not packed.is_cuda or packed.dtype != (torch.uint8 if bf16 else torch.float32):
        raise RuntimeError(f"{what}: packed must be the device image of "
                           f"{'wavenet_bf16_pack_weights' if bf16 else 'wavenet_pack_weights'}")
    _require_frames(frames, desc.batch, what)
    assert tuple(x.shape) == (desc.batch, desc.residual_channels, desc.t) and x.is_contiguous(), tuple(x.shape)
    assert tuple(c.shape) == (desc.batch, desc.aux_channels, desc.t) and c.is_contiguous(), tuple(c.shape)
    for t in (skips, skips_out, x_out):
        assert t is None or (t.shape == x.shape and t.is_contiguous())
    if x_out is None:
        x_out = torch.empty_like(x)
    if skips_out is None:
        skips_out = torch.empty_like(x)
    args = [ctypes.byref(desc), _ptr(x), _ptr(c), _ptr(skips), _ptr(packed), _ptr(b_dil), _ptr(b_skip), _ptr(b_out),
            _ptr(x_out), _ptr(skips_out)]
    if bf16:
        rc = _lib.lib().pwg_wavenet_bf16_layer_forward_ragged(*args, int(mfma_shape or 0), _ptr(frames), int(rate),
                                                              _stream())
    else:
        rc = _lib.lib().pwg_wavenet_layer_forward_ragged(*args, _ptr(frames), int(rate), _stream())
    _lib.check(rc, what)
    return x_out, skips_out


def wavenet_stream_bf16_supported(desc):
    """Does the bf16-operand streaming form of the causal layer (csrc/wavenet_stream_bf16.hip) cover this geometry?  The
    answer and the reason in ``_lib.lib().pwg_last_error()`` are those of :func:`wavenet_stream_supported`.  Host logic
    only."""
    return bool(_lib.lib().pwg_wavenet_stream_bf16_supported(ctypes.byref(desc)))


def wavenet_stream_delayed_bf16_supported(desc, c_delay=0):
    """Does the bf16-operand delayed form (csrc/wavenet_stream_bf16.hip) cover this geometry with the conditioning read
    ``c_delay`` columns late?  The answer and the reason are those of :func:`wavenet_stream_delayed_supported`.  Host
    logic only."""
    return bool(_lib.lib().pwg_wavenet_stream_bf16_delayed_supported(ctypes.byref(desc), int(c_delay)))


def _bf16_stream_image(name, packed):
    if not packed.is_cuda or packed.dtype != torch.uint8:
        raise RuntimeError(f"{name}: packed must be the device image of wavenet_bf16_pack_weights")


def wavenet_stream_forward_bf16(desc, x, c, skips, hist_in, hist_out, packed, b_dil, b_skip, b_out, skips_out=None,
                                save=False):
    """:func:`wavenet_stream_forward` with bf16 operands on the image of :func:`wavenet_bf16_pack_weights` -> (x_out,
    skips_out), with ``save`` (stage tests) -> (x_out, skips_out, z, g): the fp32 ``z`` and the bf16-rounded gate output
    (stored as fp32).  ``hist_out`` receives the same raw fp32 columns as in fp32."""
    return _wavenet_stream(_lib.lib().pwg_wavenet_stream_bf16_forward, "wavenet_stream_forward_bf16", desc, x, c, skips,
                           hist_in, hist_out, packed, b_dil, b_skip, b_out, bf16=True, skips_out=skips_out, save=bool(save))


def wavenet_stream_delayed_forward_bf16(desc, x, c, c_line, c_delay, skips, skip_line, hist_in, hist_out, packed, b_dil,
                                        b_skip, b_out, valid=None, save=False):
    """:func:`wavenet_stream_delayed_forward` with bf16 operands on the image of :func:`wavenet_bf16_pack_weights` ->
    (x_out, skips_out), with ``save`` (stage tests) -> (x_out, skips_out, z, g); ``z`` and ``g`` are not masked by the
    valid window.  The history and the skip line receive the same raw fp32 columns as in fp32."""
    return _wavenet_stream(_lib.lib().pwg_wavenet_stream_bf16_delayed_forward, "wavenet_stream_delayed_forward_bf16", desc,
                           x, c, skips, hist_in, hist_out, packed, b_dil, b_skip, b_out, bf16=True,
                           delayed=(c_line, c_delay, skip_line), valid=valid, save=bool(save))


def wavenet_pack_weights_bwd(desc, w_dil, s_dil, w_aux, s_aux, w_skip, s_skip, w_out, s_out):
    """Backward-pass image of a layer (gate / dilated / aux data gradients; folds desc.out_mul and desc.skip_mul)."""
    _require_device(w_dil, s_dil, w_aux, s_aux, w_skip, s_skip, w_out, s_out)
    out = torch.empty(_lib.lib().pwg_wavenet_packed_weight_bwd_floats(ctypes.byref(desc)), device=w_dil.device,
                      dtype=torch.float32)
    _lib.check(_lib.lib().pwg_wavenet_pack_weights_bwd(ctypes.byref(desc), _ptr(w_dil), _ptr(s_dil), _ptr(w_aux), _ptr(s_aux),
                                                       _ptr(w_skip), _ptr(s_skip), _ptr(w_out), _ptr(s_out), _ptr(out),
                                                       _stream()), "wavenet_pack_weights_bwd")
    return out


def wavenet_gate_backward(desc, z, dx_out, ds_out, packed_bwd):
    """(dz, go): gradient w.r.t. the gate input and the scaled residual-path gradient ``out_mul * dx_out`` (None
    when ``dx_out`` is None)."""
    _require_device(z, dx_out, ds_out, packed_bwd)
    dz = torch.empty_like(z)
    go = None if dx_out is None else torch.empty_like(dx_out)
    _lib.check(_lib.lib().pwg_wavenet_gate_backward(ctypes.byref(desc), _ptr(z), _ptr(dx_out), _ptr(ds_out),
                                                    _ptr(packed_bwd), _ptr(dz), _ptr(go), _stream()), "wavenet_gate_backward")
    return dz, go


def wavenet_data_backward(desc, dz, go, packed_bwd, need_dx=True, need_dc=True, dc_accum=None):
    """(dx, dc) = data gradients of the dilated convolution (+ go) and of the aux 1x1 convolution (+ ``dc_accum``:
    what the later layers already accumulated for the shared aux features)."""
    _require_device(dz, go, packed_bwd, dc_accum)
    b, t = dz.shape[0], dz.shape[2]
    dx = torch.empty((b, desc.residual_channels, t), device=dz.device, dtype=torch.float32) if need_dx else None
    dc = torch.empty((b, desc.aux_channels, t), device=dz.device, dtype=torch.float32) if need_dc else None
    if dx is None and dc is None:
        return None, None
    if dc_accum is not None and (tuple(dc_accum.shape) != (b, desc.aux_channels, t) or not dc_accum.is_contiguous()):
        raise ValueError("wavenet_data_backward: dc_accum must be a contiguous (B, aux, T) tensor")
    _lib.check(_lib.lib().pwg_wavenet_data_backward(ctypes.byref(desc), _ptr(dz), _ptr(go), _ptr(packed_bwd), _ptr(dc_accum),
                                                    _ptr(dx), _ptr(dc), _stream()), "wavenet_data_backward")
    return dx, dc


def wavenet_weight_backward_plan(desc):
    """How the two contraction launches of ``wavenet_weight_backward`` slice the flattened (item, 32-column chunk) range
    (host only: no launch, no device needed): dict(slices=(dil+aux, skip+out), chunks_per_slice=(dil+aux, skip+out)).
    An unsupported descriptor raises with the library's reason."""
    out = (ctypes.c_int32 * 4)()
    _lib.check(_lib.lib().pwg_wavenet_weight_backward_plan(ctypes.byref(desc), out), "wavenet_weight_backward_plan")
    return dict(slices=(out[0], out[2]), chunks_per_slice=(out[1], out[3]))


def wavenet_weight_backward(desc, dz, x, c, gs, go, g, convs=None):
    """Parameter gradients of the layer's four convolutions (csrc/wavenet.hip: two contraction launches + one finish
    launch).  ``convs`` = four ``(v, g, has_bias)`` entries (dilated, aux, skip, out): ``v``/``g`` the weight-norm
    tensors or None for a plain weight.  Returns four ``(dw_or_dv, dg, db)`` tuples in torch layouts
    ((128,64,3), (128,aux,1), (64,64,1), (64,64,1)); the last is (None, None, None) when ``go`` is None (the
    layer's residual output is unused)."""
    if convs is None:
        convs = ((None, None, True), (None, None, False), (None, None, True), (None, None, True))
    _require_device(dz, x, c, gs, go, g, *[t for cv in convs for t in cv[:2]])
    dev = dz.device
    r, gch, sch, aux = desc.residual_channels, desc.gate_channels, desc.skip_channels, desc.aux_channels
    shapes = ((gch, r, desc.kernel), (gch, aux, 1), (sch, r, 1), (r, r, 1))
    arr = (_lib.WaveNetParamGrad * 4)()
    outs = []
    for i, ((v, gg, has_b), shp) in enumerate(zip(convs, shapes)):
        if i == 3 and go is None:
            outs.append((None, None, None))
            continue
        if v is not None and (tuple(v.shape) != shp or gg is None or gg.numel() != shp[0] or not v.is_contiguous()
                              or not gg.is_contiguous()):
            raise ValueError(f"wavenet_weight_backward: conv {i}: weight-norm tensors do not match {shp}")
        dw = torch.empty(shp, device=dev, dtype=torch.float32)
        dg = torch.empty_like(gg) if v is not None else None
        db = torch.empty(shp[0], device=dev, dtype=torch.float32) if has_b else None
        arr[i].v, arr[i].g, arr[i].dw, arr[i].dg, arr[i].db = _ptr(v), _ptr(gg), _ptr(dw), _ptr(dg), _ptr(db)
        outs.append((dw, dg, db))
    n = _lib.lib().pwg_wavenet_weight_backward_workspace_floats(ctypes.byref(desc))
    if n == 0:
        _lib.check(-1, "wavenet_weight_backward_workspace_floats")
    ws = torch.empty(n, device=dev, dtype=torch.float32)
    _lib.check(_lib.lib().pwg_wavenet_weight_backward(ctypes.byref(desc), _ptr(dz), _ptr(x), _ptr(c), _ptr(gs), _ptr(go),
                                                      _ptr(g), arr, _ptr(ws), n, _stream()), "wavenet_weight_backward")
    return outs


def pack_weight_bwd(desc, w, scale=None):
    """Weight image for the data-gradient direction of ``desc`` (forward descriptor)."""
    _require_device(w, scale)
    n = _lib.lib().pwg_conv1d_packed_weight_bwd_floats(ctypes.byref(desc))
    if n == 0:
        _lib.check(-1, "packed_weight_bwd_floats")
    out = torch.empty(n, device=w.device, dtype=torch.float32)
    _lib.check(_lib.lib().pwg_conv1d_pack_weight_bwd(ctypes.byref(desc), _ptr(w), _ptr(scale), _ptr(out), _stream()),
               "conv1d_pack_weight_bwd")
    return out


def conv1d_backward_data(desc, dy, w_packed_bwd, x=None, accum=None, out=None):
    """dx = pre_act'(x) * data_grad(dy) (+ accum); ``desc`` is the forward descriptor."""
    _require_device(dy, w_packed_bwd, x, accum, out)
    if out is None:
        out = torch.empty((desc.batch, desc.c_in, desc.t_in * desc.width), device=dy.device, dtype=torch.float32)
    ws, ws_n = _workspace(_lib.lib().pwg_conv1d_backward_data_workspace_floats(ctypes.byref(desc)), dy.device)
    _lib.check(_lib.lib().pwg_conv1d_backward_data(ctypes.byref(desc), _ptr(dy), _ptr(w_packed_bwd), _ptr(x),
                                                   _ptr(accum), _ptr(out), _ptr(ws), ws_n, _stream()),
               "conv1d_backward_data")
    return out


def conv1d_backward_weight(desc, x, dy, weight_shape, need_dw=True, need_db=True, out_dw=None, out_db=None):
    """(dw in torch layout, db); deterministic two-stage reduction over (batch, time) slices.  ``out_dw`` / ``out_db``:
    optional destinations (contiguous, the right number of elements), e.g. data-parallel bucket slots."""
    _require_device(x, dy, out_dw, out_db)
    dw = (out_dw if out_dw is not None else torch.empty(weight_shape, device=x.device, dtype=torch.float32)) if need_dw else None
    db = (out_db if out_db is not None else torch.empty(desc.c_out, device=x.device, dtype=torch.float32)) if need_db else None
    ws, ws_n = None, 0
    if need_dw:
        ws_n = _lib.lib().pwg_conv1d_backward_weight_workspace_floats(ctypes.byref(desc))
        if ws_n:
            ws = torch.empty(ws_n, device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().pwg_conv1d_backward_weight(ctypes.byref(desc), _ptr(x), _ptr(dy), _ptr(dw), _ptr(db),
                                                     _ptr(ws), ws_n, _stream()), "conv1d_backward_weight")
    return dw, db


def conv1d_backward_weight_wn(desc, x, dy, v, g, need_db=True, out_dv=None, out_dg=None, out_db=None):
    """(dv, dg, db) of a weight-normalised layer: weight-gradient kernel + ONE fused finishing kernel (slab sum
    + weight-norm backward); ``v`` is weight_v in torch layout, ``g`` weight_g.  ``out_*``: optional destinations."""
    _require_device(x, dy, v, g, out_dv, out_dg, out_db)
    dv = out_dv if out_dv is not None else torch.empty_like(v)
    dg = out_dg if out_dg is not None else torch.empty_like(g)
    db = (out_db if out_db is not None else torch.empty(desc.c_out, device=x.device, dtype=torch.float32)) if need_db else None
    ws_n = _lib.lib().pwg_conv1d_backward_weight_wn_workspace_floats(ctypes.byref(desc))
    ws = torch.empty(max(ws_n, 1), device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().pwg_conv1d_backward_weight_wn(ctypes.byref(desc), _ptr(x), _ptr(dy), _ptr(v), _ptr(g), _ptr(dv),
                                                        _ptr(dg), _ptr(db), _ptr(ws), ws_n, _stream()),
               "conv1d_backward_weight_wn")
    return dv, dg, db


def weight_norm_scale(v, g):
    """scale[i] = g[i] / ||v[i]||  (old-style weight_norm, dim=0)."""
    _require_device(v, g)
    n0 = v.shape[0]
    inner = v.numel() // n0
    scale = torch.empty(n0, device=v.device, dtype=torch.float32)
    _lib.check(_lib.lib().pwg_weight_norm_scale(_ptr(v), _ptr(g), _ptr(scale), n0, inner, _stream()), "weight_norm_scale")
    return scale


def scale_rows(v, scale):
    _require_device(v, scale)
    n0 = v.shape[0]
    inner = v.numel() // n0
    w = torch.empty_like(v)
    _lib.check(_lib.lib().pwg_scale_rows(_ptr(v), _ptr(scale), _ptr(w), n0, inner, _stream()), "scale_rows")
    return w


def conv1d_forward_cfg(desc, x, w_packed, bias=None, add1=None, add2=None, out=None, tile_config=0, use_dma=True):
    """Tuning entry: explicit tile configuration / staging path (see include/pwg_kernels.h)."""
    _require_device(x, w_packed, bias, add1, add2, out)
    if out is None:
        out = torch.empty((desc.batch, desc.c_out, desc.t_out * desc.width), device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().pwg_conv1d_forward_cfg(ctypes.byref(desc), _ptr(x), _ptr(w_packed), _ptr(bias), _ptr(add1),
                                                 _ptr(add2), _ptr(out), int(tile_config), int(bool(use_dma)),
                                                 _stream()), "conv1d_forward_cfg")
    return out


def num_tile_configs():
    return _lib.lib().pwg_conv1d_num_tile_configs()


PLAN_FAMILIES = ("mfma", "grouped", "single_input_channel", "few_output_channels")


def conv1d_plan(desc, has_addends=False):
    """The launch plan ``pwg_conv1d_forward`` derives for ``desc`` (host only: no launch, no device needed):
    dict(family, tile_config, ksplit, dma, item_major, grid)."""
    out = (ctypes.c_int32 * 8)()
    _lib.check(_lib.lib().pwg_conv1d_plan(ctypes.byref(desc), int(bool(has_addends)), out), "conv1d_plan")
    return dict(family=PLAN_FAMILIES[out[0]], tile_config=out[1], ksplit=out[2], dma=bool(out[3]),
                item_major=bool(out[4]), grid=(out[5], out[6], out[7]))


WGRAD_PATHS = ("mfma", "gconv", "small_cin", "k1")
WGRAD_FINISHERS = ("direct", "slabs", "slabs_wide", "wn_two_kernel", "wn_fused", "wn_fused_wide")


def conv1d_wgrad_plan(desc, weight_norm=False, has_bias=True):
    """What ``conv1d_backward_weight`` (``weight_norm=True``: ``conv1d_backward_weight_wn``) launches for ``desc`` (host
    only: no launch, no device needed): dict(path, finisher, workspace_floats, slabs) and, for the ``mfma`` path,
    small, tg, taps_block, tap_groups, win, tt, rows_half, rows_x4, mode, act, stride_ct, tiles, splits, lds, xs_stride."""
    out = (ctypes.c_int32 * 20)()
    _lib.check(_lib.lib().pwg_conv1d_backward_weight_plan(ctypes.byref(desc), int(bool(weight_norm)), int(bool(has_bias)),
                                                          out), "conv1d_backward_weight_plan")
    plan = dict(path=WGRAD_PATHS[out[0]], finisher=WGRAD_FINISHERS[out[1]], workspace_floats=out[2] + (out[3] << 31),
                slabs=out[18])
    if plan["path"] == "mfma":
        plan.update(small=bool(out[4]), tg=out[5], taps_block=out[6], tap_groups=out[7], win=bool(out[8]), tt=out[9],
                    rows_half=out[10], rows_x4=bool(out[11]), mode=out[12], act=bool(out[13]), stride_ct=out[14],
                    tiles=out[15], splits=out[16], lds=out[17], xs_stride=out[19])
    return plan


def conv_tile_of_workgroup(grid, row_blocks, ksplit, item_major, workgroup):
    """Host evaluation of the convolution kernel's dispatch-id -> logical-tile map (column tile, row block index,
    item * ksplit + slice)."""
    out = (ctypes.c_int32 * 3)()
    _lib.check(_lib.lib().pwg_debug_conv_tile_of_workgroup(int(grid[0]), int(grid[1]), int(grid[2]), int(row_blocks),
                                                           int(ksplit), int(bool(item_major)), int(workgroup), out),
               "conv_tile_of_workgroup")
    return out[0], out[1], out[2]


class profile:
    """Context manager: per-kernel-family HIP-event timing of every launch made through the
    C ABI (``pwg_prof_*``).  ``.results`` -> {kernel: dict(ms, launches, flops, bytes)}."""

    def __enter__(self):
        l = _lib.lib()
        l.pwg_prof_reset()
        l.pwg_prof_enable(1)
        self.results = {}
        return self

    def __exit__(self, *exc):
        l = _lib.lib()
        l.pwg_prof_enable(0)
        n = l.pwg_prof_num_kernels()
        for i in range(n):
            name = ctypes.create_string_buffer(256)
            ms, fl, by = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
            cnt = ctypes.c_int64()
            _lib.check(l.pwg_prof_get(i, name, 256, ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(fl),
                                      ctypes.byref(by)), "prof_get")
            self.results[name.value.decode()] = dict(ms=ms.value, launches=cnt.value, flops=fl.value, bytes=by.value)
        l.pwg_prof_reset()
        return False
