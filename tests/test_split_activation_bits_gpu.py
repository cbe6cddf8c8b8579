"""GPU: the activation in front of the 3-way split, and the edge tiles' staging, bit for bit.

Every staging and forming site of csrc/conv1d_split.hip and csrc/resunit_split.hip activates a value with one of the two
forms of csrc/mfma_conv.h -- ``SplitActLeaky`` (leaky with 0 < slope < 1: ``max(v, v * slope)``) or ``SplitActMasked``
(none, relu, any other slope) -- and then splits it.  Both must give the bits of ``torch.where(x > 0, x, x * slope)``
formed in fp32, so a launch with the fused pre-activation on ``x`` must equal, by ``torch.equal``, the launch without a
pre-activation on the activated tensor; the units and the chained block, which have no launch without an activation,
must equal the chain of such convolutions that defines them (the activations between them formed by torch).

Inputs: +-0, both signs, magnitudes 2^-20 .. 2^20 and values near 2^-119, whose residuals after the bf16 head are
subnormal or zero (v * slope itself stays normal for the slopes used).  Shapes: batch 2; C 32 / 40 / 64 / 128 (a channel
tail, one to four chunks); k 3 / 7 / 11; dilation 1 / 5; T = 4, 100 (every tile an edge tile), 260 (a second tile) and
101 (T % 4 != 0: the 4-byte staging).  Each form of the step and of the window is forced where the launch admits it.

The edge identity: a row whose first and last tiles are edge tiles (checked loads from clamped addresses, zeroed by a
select) and whose middle tiles are interior equals the same signal in the middle of a longer zero-padded row."""
import functools

import pytest
import torch

from parallelwavegan_amd import _lib, ops

pytestmark = pytest.mark.gpu

B = 2
LENGTHS = (4, 100, 260, 101)
KD = [(k, d) for k in (3, 7, 11) for d in (1, 5)]
# (pre_act, slope): the leaky form at two slopes; the masked form for relu, for none and for a slope outside (0, 1)
KINDS = [("leaky_relu", 0.1), ("leaky_relu", 0.2), ("relu", 0.0), (None, 0.0), ("leaky_relu", 1.5)]


@functools.lru_cache(maxsize=None)
def _signal(c, t, seed=0):
    """CPU float32 (B, c, t): both signs, magnitudes 2^-20 .. 2^20, and at fixed places +-0 and values near 2^-119."""
    g = torch.Generator().manual_seed(7919 * c + 31 * t + seed)
    e = torch.randint(-20, 21, (B, c, t), generator=g).float()
    x = torch.randn(B, c, t, generator=g) * torch.exp2(e)
    flat = x.view(-1)
    n = flat.numel()
    flat[0::7] = 0.0
    flat[3::14] = -0.0
    tiny = (1 + torch.rand(n, generator=g)) * 2.0 ** -119
    flat[5::11] = tiny[5::11]
    flat[6::22] = -tiny[6::22]
    return x


def _activate(x, kind, slope):
    """The definition, in fp32: one rounded product, no fused multiply."""
    if kind == "leaky_relu":
        return torch.where(x > 0, x, x * slope)
    if kind == "relu":
        return torch.where(x > 0, x, torch.zeros_like(x))
    return x


@functools.lru_cache(maxsize=None)
def _weight(cout, cin, k, seed=0):
    g = torch.Generator().manual_seed(1009 * cout + 101 * cin + k + seed)
    return torch.randn(cout, cin, k, generator=g) / (cin * k) ** 0.5, torch.randn(cout, generator=g)


def _forms(t):
    """(step_form, window_form) to force: the plan's choice, both steps, and the prefetched window (16-B staging)."""
    forms = [(0, 0), (1, 0), (2, 0)]
    return forms + [(1, 2)] if t % 4 == 0 else forms


def _conv(desc, x, ws, bias, step, window):
    try:
        return ops.conv1d_forward_split(desc, x, ws, bias, step_form=step, window_form=window)
    except RuntimeError as e:  # a window the prefetched form does not cover: not a form of this launch
        if window == 2 and "prefetched window" in str(e):
            return None
        raise


@pytest.mark.parametrize("c", (32, 40, 64, 128))
@pytest.mark.parametrize("k", (3, 7, 11))
def test_conv_pre_activation_bits(c, k, device):
    w, bias = _weight(c, c, k)
    w, bias = w.to(device), bias.to(device)
    ran = 0
    for d in (1, 5):
        pad = (k - 1) // 2 * d
        for t in LENGTHS:
            x = _signal(c, t)
            xd = x.to(device)
            plain = ops.make_conv_desc(B, c, c, t, t, k, dilation=d, pad_left=pad)
            ws = ops.pack_weight_split(plain, w)
            for kind, slope in KINDS:
                fused = ops.make_conv_desc(B, c, c, t, t, k, dilation=d, pad_left=pad, pre_act=kind, pre_slope=slope)
                xa = _activate(x, kind, slope).to(device)
                for step, window in _forms(t):
                    got = _conv(fused, xd, ws, bias, step, window)
                    if got is None:
                        continue
                    want = _conv(plain, xa, ws, bias, step, window)
                    assert torch.isfinite(got).all()
                    assert torch.equal(got, want), (f"C{c} k{k} d{d} T{t} {kind} {slope} step {step} window {window}: "
                                                    f"{int((got != want).sum())} values differ")
                    ran += 1
    assert ran >= len(KINDS) * len(LENGTHS) * 2 * 3


@pytest.mark.parametrize("c", (32, 40, 64, 128))
@pytest.mark.parametrize("stride", (2, 4))
def test_transposed_pre_activation_bits(c, stride, device):
    k, pad = 2 * stride, stride // 2
    g = torch.Generator().manual_seed(c * 13 + stride)
    w = (torch.randn(c, c, k, generator=g) / (2 * c) ** 0.5).to(device)
    bias = torch.randn(c, generator=g).to(device)
    for t in LENGTHS:
        t_out = ops.conv_transpose_out_length(t, k, stride, pad, 0)
        x = _signal(c, t)
        xd = x.to(device)
        plain = ops.make_conv_desc(B, c, c, t, t_out, k, stride=stride, pad_left=pad, transposed=True)
        ws = ops.pack_weight_split_transposed(plain, w)
        for kind, slope in KINDS:
            fused = ops.make_conv_desc(B, c, c, t, t_out, k, stride=stride, pad_left=pad, transposed=True, pre_act=kind,
                                       pre_slope=slope)
            got = ops.conv1d_forward_split_transposed(fused, xd, ws, bias)
            want = ops.conv1d_forward_split_transposed(plain, _activate(x, kind, slope).to(device), ws, bias)
            assert torch.isfinite(got).all()
            assert torch.equal(got, want), f"C{c} s{stride} T{t} {kind} {slope}: {int((got != want).sum())} values differ"


def _unit_chain(x, k, d, s1, s2, i1, b1, i2, b2, device):
    """The unit by its definition: two split convolutions WITHOUT a fused pre-activation, the activations by torch."""
    b, c, t = x.shape
    c1 = ops.make_conv_desc(b, c, c, t, t, k, dilation=d, pad_left=(k - 1) // 2 * d)
    c2 = ops.make_conv_desc(b, c, c, t, t, k, dilation=1, pad_left=(k - 1) // 2)
    h = ops.conv1d_forward_split(c1, _activate(x, "leaky_relu", s1), i1, b1)
    return ops.conv1d_forward_split(c2, _activate(h, "leaky_relu", s2), i2, b2, x)


UNIT_SLOPES = ((0.1, 0.1), (0.2, 0.3))


@pytest.mark.parametrize("c", (32, 64))
@pytest.mark.parametrize("k", (3, 7, 11))
def test_unit_activation_bits(c, k, device):
    (w1, b1), (w2, b2) = _weight(c, c, k, 1), _weight(c, c, k, 2)
    wdesc = ops.make_conv_desc(1, c, c, 64, 64, k, pad_left=(k - 1) // 2)
    i1, i2 = ops.pack_weight_split(wdesc, w1.to(device)), ops.pack_weight_split(wdesc, w2.to(device))
    b1, b2 = b1.to(device), b2.to(device)
    for d in (1, 5):
        for t in (4, 100, 260):
            x = _signal(c, t).to(device)
            for s1, s2 in UNIT_SLOPES:
                desc = ops.make_resunit_desc(B, c, t, k, d, True, s1, s2)
                got = ops.resunit_forward_split(desc, x, i1, b1, i2, b2)
                want = _unit_chain(x, k, d, s1, s2, i1, b1, i2, b2, device)
                assert torch.isfinite(got).all()
                assert torch.equal(got, want), f"C{c} k{k} d{d} T{t} slopes {s1} {s2}: {int((got != want).sum())} differ"


@pytest.mark.parametrize("c,k", [(32, 3), (64, 3), (32, 7)])
def test_block_activation_bits(c, k, device):
    dil, s1, s2 = (1, 5), (0.1, 0.2), (0.2, 0.1)
    wdesc = ops.make_conv_desc(1, c, c, 64, 64, k, pad_left=(k - 1) // 2)
    ws = [[_weight(c, c, k, 10 * u + j) for j in (1, 2)] for u in range(2)]
    i1 = [ops.pack_weight_split(wdesc, ws[u][0][0].to(device)) for u in range(2)]
    i2 = [ops.pack_weight_split(wdesc, ws[u][1][0].to(device)) for u in range(2)]
    b1 = [ws[u][0][1].to(device) for u in range(2)]
    b2 = [ws[u][1][1].to(device) for u in range(2)]
    for t in (4, 100, 260):
        x = _signal(c, t).to(device)
        desc = ops.make_resunit_desc(B, c, t, k, 1, True, s1[0], s2[0])
        assert ops.resblock_split_supported(desc, dil), _lib.lib().pwg_last_error().decode()
        got = ops.resblock_forward_split(desc, x, dil, s1, s2, i1, b1, i2, b2)
        want = x
        for u in range(2):
            want = _unit_chain(want, k, dil[u], s1[u], s2[u], i1[u], b1[u], i2[u], b2[u], device)
        assert torch.isfinite(got).all()
        assert torch.equal(got, want), f"C{c} k{k} T{t}: {int((got != want).sum())} values differ"


@pytest.mark.parametrize("step", (0, 1, 2))
def test_edge_tiles_equal_the_middle_of_a_padded_row(step, device):
    """C = 64, T = 1024, k = 11, d = 5: eight column tiles, the first and the last checked, the others interior.  In a
    row with 260 zeros on each side the same samples are staged by interior tiles at other tile offsets."""
    c, t, k, d, margin = 64, 1024, 11, 5, 260
    pad = (k - 1) // 2 * d
    w, bias = _weight(c, c, k, 3)
    x = _signal(c, t, 3)
    wide = torch.zeros(B, c, t + 2 * margin)
    wide[:, :, margin:margin + t] = x
    short = ops.make_conv_desc(B, c, c, t, t, k, dilation=d, pad_left=pad, pre_act="leaky_relu", pre_slope=0.1)
    long = ops.make_conv_desc(B, c, c, wide.shape[2], wide.shape[2], k, dilation=d, pad_left=pad, pre_act="leaky_relu",
                              pre_slope=0.1)
    ws = ops.pack_weight_split(short, w.to(device))
    bias = bias.to(device)
    for mode in (0, 1, 2):
        got = ops.conv1d_forward_split(short, x.to(device), ws, bias, tile_mode=mode, step_form=step)
        want = ops.conv1d_forward_split(long, wide.to(device), ws, bias, tile_mode=mode, step_form=step)
        want = want[:, :, margin:margin + t]
        assert torch.equal(got, want), f"tile_mode {mode}: {int((got != want).sum())} values differ"
