"""The rule of the ragged StyleMelGAN forward in plain torch, any dtype, on the CPU: every item's
instance-norm statistics run over its own columns ``[0, e)`` and every layer leaves exact zeros from ``e`` on, so the
zero-padded convolutions read past an item's end what they read past the end of the item alone.  The layers are
``oracle.torch_cpu``'s (``tade_layer`` / ``tade_res_block`` / ``style_melgan_generator``) with the two changes, nothing
else; in float64 this equals the oracle on each item alone to rounding, which proves the rule before any kernel runs.

Also the inputs the StyleMelGAN ragged tests share: the items, their segment counts and the padded batch."""
import torch
import torch.nn.functional as F

from oracle.torch_cpu import get_bias, get_weight
from tests.golden import synth

SEED, G_SCALE = 11, 1.1
FRAMES = (19, 7, 12, 3, 0)  # frames per item; the last item is unused


def segments_of(frames, segment_frames):
    return tuple(-(-n // segment_frames) for n in frames)


def zero_tail(x, ends):
    """Exact zeros at the columns >= ends[b] of item b (a copy)."""
    x = x.clone()
    for b, e in enumerate(ends):
        x[b, :, e:] = 0.0
    return x


def instance_norm(x, ends, eps=1e-5):
    """InstanceNorm1d(affine=False) with each item's statistics over [0, ends[b]); zeros from there on."""
    y = torch.zeros_like(x)
    for b, e in enumerate(ends):
        if e > 0:
            seg = x[b, :, :e]
            mu = seg.mean(dim=1, keepdim=True)
            var = ((seg - mu) ** 2).mean(dim=1, keepdim=True)  # biased
            y[b, :, :e] = (seg - mu) / torch.sqrt(var + eps)
    return y


def _conv(sd, p, x, dilation=1):
    w = get_weight(sd, p)
    return F.conv1d(x, w, get_bias(sd, p), dilation=dilation, padding=(w.shape[-1] - 1) // 2 * dilation)


def tade_layer(sd, prefix, x, c, ends, f):
    up = [e * f for e in ends]
    xn = instance_norm(x, ends)
    c = F.interpolate(c, scale_factor=f, mode="nearest") if f != 1 else c
    c = zero_tail(_conv(sd, prefix + ".aux_conv.0", c), up)
    cg1, cg2 = _conv(sd, prefix + ".gated_conv.0", c).chunk(2, dim=1)
    xu = F.interpolate(xn, scale_factor=f, mode="nearest") if f != 1 else xn
    return zero_tail(cg1 * xu + cg2, up), c


def tade_res_block(sd, prefix, x, c, ends, f, dilation, gated_function):
    def gate(v, e):
        va, vb = v.chunk(2, dim=1)
        g = torch.softmax(va, dim=1) if gated_function == "softmax" else torch.sigmoid(va)
        return zero_tail(g * torch.tanh(vb), e)

    up = [e * f for e in ends]
    residual = x
    x, c = tade_layer(sd, prefix + ".tade1", x, c, ends, 1)
    x = gate(_conv(sd, prefix + ".gated_conv1", x), ends)
    x, c = tade_layer(sd, prefix + ".tade2", x, c, ends, f)
    x = gate(_conv(sd, prefix + ".gated_conv2", x, dilation), up)
    ru = F.interpolate(residual, scale_factor=f, mode="nearest") if f != 1 else residual
    return zero_tail(ru + x, up), c, up


def ragged_generator(sd, c, z, segments, noise_upsample_scales=(11, 2, 2, 2), upsample_scales=(2, 2, 2, 2, 2, 2, 2, 2, 1),
                     dilation=2, gated_function="softmax", noise_slope=0.2, **_unused):
    """c (B, aux, S_max * F), z (B, in_channels, S_max), segments: ints per item -> (B, out, S_max * F * up)."""
    ends = [int(s) for s in segments]
    x = zero_tail(z, ends)
    for i, s in enumerate(noise_upsample_scales):
        p = f"noise_upsample.{2 * i}"
        ends = [e * s for e in ends]
        x = zero_tail(F.leaky_relu(F.conv_transpose1d(x, get_weight(sd, p), get_bias(sd, p), stride=s,
                                                      padding=s // 2 + s % 2, output_padding=s % 2), noise_slope), ends)
    c = zero_tail(c, ends)
    for i, s in enumerate(upsample_scales):
        x, c, ends = tade_res_block(sd, f"blocks.{i}", x, c, ends, s, dilation, gated_function)
    return zero_tail(torch.tanh(_conv(sd, "output_conv.0", x)), ends)


# ---- the inputs the host and the GPU tests share
def items(cfg, frames=FRAMES, seed=SEED):
    """Per item (features (T, aux), noise (in_channels, ceil(T / F))), float32; an unused item has 0 rows / columns."""
    sf = 1
    for s in cfg["noise_upsample_scales"]:
        sf *= s
    return [(synth.synth_input(f"c{j}", (n, cfg["aux_channels"]), seed=seed),
             synth.synth_input(f"z{j}", (cfg["in_channels"], -(-n // sf)), seed=seed)) for j, n in enumerate(frames)]


def alone_inputs(feat, noise, segment_frames):
    """What ``inference`` runs for one utterance: c (1, aux, S * F), the last frame replicated, and z (1, in, S)."""
    c = feat.t().unsqueeze(0)
    return F.pad(c, (0, noise.shape[1] * segment_frames - c.shape[2]), mode="replicate").contiguous(), noise.unsqueeze(0)


def padded_batch(its, segment_frames, s_max, fill=0.0):
    """The batch (c (B, aux, S_max * F), z (B, in, S_max)): each item's ``alone_inputs`` first, ``fill`` behind."""
    aux, cin = its[0][0].shape[1], its[0][1].shape[0]
    c = torch.full((len(its), aux, s_max * segment_frames), fill)
    z = torch.full((len(its), cin, s_max), fill)
    for j, (feat, noise) in enumerate(its):
        if feat.shape[0]:
            cj, zj = alone_inputs(feat, noise, segment_frames)
            c[j, :, :cj.shape[2]], z[j, :, :zj.shape[2]] = cj[0], zj[0]
    return c, z
