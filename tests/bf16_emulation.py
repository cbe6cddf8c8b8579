"""CPU emulation of the bf16-operand inference mode (test infrastructure).

The mode's numerical definition (include/pwg_kernels.h, csrc/conv1d_bf16.hip): the input of a convolution -- after its
pre-activation, which the CPU oracle applies before it calls the convolution -- and the effective fp32 weight are rounded
to bf16 (round-to-nearest-even); products are accumulated in fp32; bias and everything after it are fp32.  Inside
``bf16_operands()`` the two functional convolutions that ``oracle/torch_cpu.py`` calls round their input and weight with
``.to(torch.bfloat16).to(torch.float32)`` before the fp32 CPU op, so any oracle function runs under that definition
without being edited.
"""
import contextlib

import torch
import torch.nn.functional as F


def round_bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


@contextlib.contextmanager
def bf16_operands(predicate=None, accumulate=None):
    """``predicate(kind, x, w, kwargs) -> bool`` decides per call whether the operands are rounded (``kind``:
    ``"conv1d"`` / ``"conv_transpose1d"``; default: always) -- it mirrors ``ops.conv1d_bf16_supported`` for mixed
    networks.  ``accumulate``: optional dtype (``torch.float64``) the rounded operands are convolved in, to measure how
    much of a difference is accumulation order.  Yields a dict counting rounded / untouched calls."""
    orig = (F.conv1d, F.conv_transpose1d)
    stats = {"rounded": 0, "untouched": 0}

    def wrap(kind, fn):
        def conv(x, w, bias=None, *args, **kwargs):
            if predicate is not None and not predicate(kind, x, w, kwargs):
                stats["untouched"] += 1
                return fn(x, w, bias, *args, **kwargs)
            stats["rounded"] += 1
            xr, wr = round_bf16(x), round_bf16(w)
            if accumulate is None:
                return fn(xr, wr, bias, *args, **kwargs)
            y = fn(xr.to(accumulate), wr.to(accumulate), None if bias is None else bias.to(accumulate), *args, **kwargs)
            return y.to(x.dtype)

        return conv

    F.conv1d, F.conv_transpose1d = wrap("conv1d", orig[0]), wrap("conv_transpose1d", orig[1])
    try:
        yield stats
    finally:
        F.conv1d, F.conv_transpose1d = orig


def rms(t):
    return float(torch.as_tensor(t).detach().cpu().double().pow(2).mean().sqrt())
