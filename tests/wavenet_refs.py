"""Plain torch references of the three data kernels of ``csrc/wavenet.hip`` (layer forward, gate backward, data
backward), written from the formulas of the layer (layers/residual_block.py:102-140 of the reference project), not
from the kernels, and importable without a GPU.  No autograd inside: the backward references are the adjoints written
out, checked against ``torch.autograd.grad`` in tests/test_wavenet_refs_host.py.

One function per kernel, each on THAT KERNEL'S OWN INPUTS, so that no stage's rounding enters the bar of a later one
(the stage-by-stage rule of tests/test_wavenet_bf16_gpu.py).  ``Wd`` (128, 64, 3), ``Wa`` (128, aux, 1), ``Ws`` and
``Wo`` (64, 64, 1) are the EFFECTIVE weights ``w * scale[:, None, None]`` (``effective``); a scale of None is 1.
Every function is dtype-generic: float64 tensors in, the reference out.
"""
import torch
import torch.nn.functional as F

D = torch.float64
HALF = 64  # gate-output channels: tanh half = z[:, :64], sigmoid half = z[:, 64:]


def effective(w, scale=None):
    """``w * scale[:, None, None]`` in float64 from the float32 values the kernel's packer reads."""
    w = w.detach().cpu().to(D)
    return w if scale is None else w * scale.detach().cpu().to(D).view(-1, 1, 1)


def gate(z):
    return torch.tanh(z[:, :HALF]) * torch.sigmoid(z[:, HALF:])


def skip_out(g, skips, Ws, b_skip, skip_mul):
    s = F.conv1d(g, Ws, b_skip)
    return (s if skips is None else s + skips) * skip_mul


def res_out(g, x, Wo, b_out, out_mul):
    return (F.conv1d(g, Wo, b_out) + x) * out_mul


def layer_forward(x, c, skips, Wd, Wa, Ws, Wo, b_dil, b_skip, b_out, dil, out_mul, skip_mul):
    """-> (z, g, skips_out, x_out); a None bias or None skips is a zero term."""
    z = F.conv1d(x, Wd, b_dil, padding=dil, dilation=dil) + F.conv1d(c, Wa)
    g = gate(z)
    return z, g, skip_out(g, skips, Ws, b_skip, skip_mul), res_out(g, x, Wo, b_out, out_mul)


def gate_backward(z, dx_out, ds_out, Ws, Wo, out_mul, skip_mul):
    """-> (dz, go); ``go = out_mul * dx_out`` is None (a zero term) when ``dx_out`` is None."""
    go = None if dx_out is None else out_mul * dx_out
    dg = F.conv_transpose1d(skip_mul * ds_out, Ws)
    if go is not None:
        dg = dg + F.conv_transpose1d(go, Wo)
    th, sg = torch.tanh(z[:, :HALF]), torch.sigmoid(z[:, HALF:])
    dz = torch.cat([dg * sg * (1 - th * th), dg * th * sg * (1 - sg)], 1)
    return dz, go


def data_backward(dz, go, Wd, Wa, dil, dc_accum):
    """-> (dx, dc); a None ``go`` or ``dc_accum`` is a zero term."""
    dx = F.conv_transpose1d(dz, Wd, padding=dil, dilation=dil)
    if go is not None:
        dx = dx + go
    dc = F.conv_transpose1d(dz, Wa)
    if dc_accum is not None:
        dc = dc + dc_accum
    return dx, dc
