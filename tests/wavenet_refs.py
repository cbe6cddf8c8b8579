"""Plain torch references of the three data kernels of ``csrc/wavenet.hip`` (layer forward, gate backward, data
backward) and of its weight path (the parameter gradients, their weight-norm backward and the per-slice slabs),
written from the formulas of the layer (layers/residual_block.py:102-140 of the reference project), not
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


# ---- the weight path (``pwg_wavenet_weight_backward``), written from its header comment in csrc/wavenet.hip and from
# include/pwg_kernels.h: two contractions over (batch, time),
#   [dW_dil | dW_aux | db_dil] = dz (128 rows)      x  [x(n - d); x(n); x(n + d); c(n)]  (272 rows), x zero outside [0, T)
#   [dW_skip ; dW_out | db]    = [gs; go] (128 rows) x  g (64 rows)
# cut into slices of ``per`` consecutive 32-column chunks of the flattened (item, chunk) range, one slab per slice
WW_COLS = 32  # columns of a chunk


def _taps(x, dil):
    """(3, B, C, T): x(n + (k - 1) dil) for k = 0, 1, 2, zero outside the sequence."""
    T = x.shape[-1]
    xp = F.pad(x, (dil, dil))
    return torch.stack([xp[:, :, k * dil:k * dil + T] for k in range(3)])


def weight_backward(dz, x, c, gs, go, g, dil):
    """-> dict dWd (128, 64, 3), dWa (128, aux, 1), db_dil (128), dWs (64, 64, 1), db_skip (64), dWo, db_out (None
    without ``go``): the gradients w.r.t. the four EFFECTIVE weights and the three biases."""
    con = lambda m, n: torch.einsum("bmt,bct->mc", m, n)  # noqa: E731
    out = dict(dWd=torch.stack([con(dz, xk) for xk in _taps(x, dil)], dim=2), dWa=con(dz, c)[:, :, None],
               db_dil=dz.sum((0, 2)), dWs=con(gs, g)[:, :, None], db_skip=gs.sum((0, 2)), dWo=None, db_out=None)
    if go is not None:
        out.update(dWo=con(go, g)[:, :, None], db_out=go.sum((0, 2)))
    return out


def weight_norm_backward(dw, v, g):
    """-> (dv, dg) of ``w = g v / |v|`` (|v| per output row) from dw: dg = <dw, v> / |v|,
    dv = (g / |v|) (dw - v <dw, v> / |v|^2); ``dg`` has the shape of ``g``."""
    rows = v.shape[0]
    col = (rows,) + (1,) * (v.dim() - 1)
    norm = (v * v).flatten(1).sum(1).sqrt().view(col)
    dot = (dw * v).flatten(1).sum(1).view(col)
    dv = (g.view(col) / norm) * (dw - v * dot / (norm * norm))
    return dv, (dot / norm).view(g.shape)


def slab_ranges(B, T, per):
    """For every slice the (item, n0, n1) column ranges it owns: the flattened (item, 32-column chunk) range in runs of
    ``per`` chunks (the last run may be shorter; a run that crosses an item boundary owns a range in each item)."""
    per_item = -(-T // WW_COLS)
    total = B * per_item
    slices = []
    for c0 in range(0, total, per):
        ranges = []
        for ch in range(c0, min(c0 + per, total)):
            b, n0 = divmod(ch, per_item)
            n0 *= WW_COLS
            n1 = min(n0 + WW_COLS, T)
            if ranges and ranges[-1][0] == b and ranges[-1][2] == n0:
                ranges[-1] = (b, ranges[-1][1], n1)
            else:
                ranges.append((b, n0, n1))
        slices.append(ranges)
    return slices


def weight_backward_slabs(dz, x, c, gs, go, g, dil, per):
    """-> (slabs0 [slices0][128][3 * 64 + aux + 1], slabs1 [slices1][128][64 + 1]) for ``per`` = (chunks per slice of the
    dil+aux launch, of the skip+out launch): per slice ``M N^T`` over the columns it owns, N = [tap0 x | tap1 x | tap2 x |
    c] resp. g, M = dz resp. [gs; go] (a None ``go`` is zero rows); the last column is the row sum of M."""
    B, _, T = dz.shape
    n0 = torch.cat(list(_taps(x, dil)) + [c], dim=1)
    m1 = torch.cat([gs, torch.zeros_like(gs) if go is None else go], dim=1)
    out = []
    for m, n, p in ((dz, n0, per[0]), (m1, g, per[1])):
        slabs = []
        for ranges in slab_ranges(B, T, p):
            slab = m.new_zeros(m.shape[1], n.shape[1] + 1)
            for b, lo, hi in ranges:
                slab[:, :-1] += m[b, :, lo:hi] @ n[b, :, lo:hi].T
                slab[:, -1] += m[b, :, lo:hi].sum(1)
            slabs.append(slab)
        out.append(torch.stack(slabs))
    return tuple(out)
