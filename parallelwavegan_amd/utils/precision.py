"""Opt-in reduced-precision inference: bf16 operands, fp32 accumulation, fp32 tensors (csrc/conv1d_bf16.hip,
csrc/wavenet_bf16.hip)."""
import contextlib

import torch

from ..layers.conv import each_conv

PRECISIONS = ("fp32", "bf16")


def set_inference_precision(model, precision):
    """Switch every convolution of ``model`` to ``"bf16"`` (bf16-operand MFMA kernel, inference only) or back to
    ``"fp32"`` (the default).  Module tree, tensor dtypes, state dicts and checkpoints do not change: the mode is an
    attribute of the convolution modules.  A convolution the bf16 kernel does not cover (grouped, (k, 1) Conv2d,
    reflect padding, strided) stays at ``"fp32"``.  Coverage is decided per block where a module runs several
    convolutions as one fused bf16 launch: a module's ``bf16_covered_convs()`` (the PWG residual block,
    csrc/wavenet_bf16.hip) names convolutions that launch covers even where the stand-alone kernel does not.  Returns how
    many convolutions took the requested mode."""
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {PRECISIONS}, got {precision!r}")
    covered = set()
    if precision == "bf16":
        for m in model.modules():
            hook = getattr(m, "bf16_covered_convs", None)
            if callable(hook):
                covered.update(id(cv) for cv in hook())
    n = 0
    for m in each_conv(model):
        if precision == "bf16" and id(m) not in covered and not m.bf16_capable():
            m.precision = "fp32"
            continue
        m.precision = precision
        n += 1
    return n


def get_inference_precision(model):
    """``"bf16"`` if any convolution of ``model`` is in bf16 mode, else ``"fp32"``."""
    return "bf16" if any(m.precision == "bf16" for m in each_conv(model)) else "fp32"


@contextlib.contextmanager
def inference_precision(model, precision):
    """``with`` block that runs ``model`` in ``precision`` and restores every convolution's own mode afterwards
    (``None``: leave the modes as they are) -- the ``precision=`` argument of the generators' ``inference()``."""
    if precision is None:
        yield
        return
    saved = [(m, m.precision) for m in each_conv(model)]
    set_inference_precision(model, precision)
    try:
        yield
    finally:
        for m, p in saved:
            m.precision = p


def no_grad_if_bf16(model):
    """``torch.no_grad()`` when any convolution of ``model`` is in bf16 mode (which has no backward pass), else a
    context that changes nothing."""
    return torch.no_grad() if get_inference_precision(model) == "bf16" else contextlib.nullcontext()
