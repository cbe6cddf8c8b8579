"""GPU: the bf16-operand one-launch WaveNet layer (csrc/wavenet_bf16.hip), stage by stage.

Every stage is compared against float64 on the kernel's OWN inputs to that stage, so that a bf16 rounding decision of an
earlier stage never enters the bar of a later one:
  z      vs the float64 convolutions of the bf16-rounded x, c and effective weights (w * scale, rounded), plus the bias;
  g      vs tanh * sigmoid of the kernel's own z in float64: every element bf16-representable and within half a bf16 ulp
         (the round-to-nearest) plus the fp32 gate bar (3e-5 of the largest value) of the fp32 kernel's test;
  x, s   vs float64 1x1 convolutions of the kernel's own g with the rounded weights, the fp32 bias, the fp32 residual /
         running skip sum and the two scales.
The product of two bf16 values is exact in fp32, so z, x and s can differ from float64 only by fp32 accumulation order:
the bar is the project's per-layer bar, 3e-5 of the largest value (test_wavenet_layer_gpu.py, test_conv_bf16_gpu.py).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from parallelwavegan_amd import ops
from tests.util import poison_empty, poison_lds

pytestmark = pytest.mark.gpu

RTOL = 3e-5
# the cases of test_wavenet_layer_gpu.py::test_layer_kernel_matches_aten
CASES = [(2, 1000, 1, False, 1.0), (1, 4096, 2, True, 1.0), (3, 777, 64, True, math.sqrt(1 / 30)),
         (2, 2048, 512, True, 1.0), (1, 50, 4, True, 1.0), (1, 640, 512, False, 1.0)]


def _bf16r(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _rel(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    return (got - want).abs().max().item() / (want.abs().max().item() + 1e-300)


def _half_ulp_bf16(v):
    """half the spacing of bf16 values at |v| (8 significant bits): 2^(e - 9) for |v| in [2^(e-1), 2^e)"""
    _, e = torch.frexp(v)
    return torch.ldexp(torch.ones_like(v), e - 9)


def _inputs(B, T, dil, with_skips):
    g = torch.Generator().manual_seed(T + dil)
    x, c = torch.randn(B, 64, T, generator=g), torch.randn(B, 80, T, generator=g)
    skips = torch.randn(B, 64, T, generator=g) if with_skips else None
    w_d = torch.randn(128, 64, 3, generator=g) / math.sqrt(192)
    w_a = torch.randn(128, 80, 1, generator=g) / math.sqrt(80)
    w_s, w_o = torch.randn(64, 64, 1, generator=g) / 8, torch.randn(64, 64, 1, generator=g) / 8
    b_d, b_s, b_o = torch.randn(128, generator=g), torch.randn(64, generator=g), torch.randn(64, generator=g)
    s_d = 1.0 + 0.2 * torch.rand(128, generator=g)  # weight-norm style row scales folded into the image
    s_o = 1.0 + 0.2 * torch.rand(64, generator=g)
    return x, c, skips, (w_d, s_d, w_a, None, w_s, None, w_o, s_o), (b_d, b_s, b_o)


def run_layer(B, T, dil, with_skips, skip_mul, device, mfma_shape=None):
    x, c, skips, ws, bs = _inputs(B, T, dil, with_skips)
    desc = ops.make_wavenet_desc(B, T, dil, out_mul=math.sqrt(0.5), skip_mul=skip_mul)
    assert ops.wavenet_bf16_supported(desc)
    d = lambda t: None if t is None else t.to(device).contiguous()  # noqa: E731
    with poison_lds(), poison_empty():
        img = ops.wavenet_bf16_pack_weights(desc, *[d(t) for t in ws])
        out = ops.wavenet_bf16_layer_forward(desc, d(x), d(c), d(skips), img, *[d(t) for t in bs], save=True,
                                             mfma_shape=mfma_shape)
    torch.cuda.synchronize()
    return (x, c, skips, ws, bs), [t.cpu() for t in out], desc


def stage_errors(inputs, out, desc):
    """(z, g, skips, x) errors of one launch, each against float64 on the kernel's own inputs to that stage."""
    (x, c, skips, ws, bs), (x_out, s_out, z_out, g_out) = inputs, out
    w_d, s_d, w_a, s_a, w_s, s_s, w_o, s_o = ws
    b_d, b_s, b_o = bs
    eff = lambda w, s: _bf16r(w if s is None else w * s.view(-1, 1, 1)).double()  # noqa: E731  (fp32 w * s, rounded)
    dil = desc.dilation
    z64 = (F.conv1d(_bf16r(x).double(), eff(w_d, s_d), b_d.double(), padding=dil, dilation=dil)
           + F.conv1d(_bf16r(c).double(), eff(w_a, s_a)))
    zk = z_out.double()
    g64 = torch.tanh(zk[:, :64]) * torch.sigmoid(zk[:, 64:])
    gk = g_out.double()
    assert torch.equal(_bf16r(g_out), g_out), "g_out holds values that are not bf16-representable"
    g_excess = ((gk - g64).abs() - _half_ulp_bf16(g64)).max().item() / g64.abs().max().item()
    s64 = (F.conv1d(gk, eff(w_s, s_s), b_s.double()) + (0.0 if skips is None else skips.double())) * desc.skip_mul
    x64 = (F.conv1d(gk, eff(w_o, s_o), b_o.double()) + x.double()) * desc.out_mul
    for name, t in (("z", z_out), ("g", g_out), ("skips", s_out), ("x", x_out)):
        assert torch.isfinite(t).all(), name
    return {"z": _rel(z_out, z64), "g_excess_over_half_ulp": g_excess, "skips": _rel(s_out, s64), "x": _rel(x_out, x64)}


@pytest.mark.parametrize("mfma_shape", [None, 32, 16])
@pytest.mark.parametrize("B,T,dil,with_skips,skip_mul", CASES)
def test_stages_match_float64(B, T, dil, with_skips, skip_mul, mfma_shape, device):
    inputs, out, desc = run_layer(B, T, dil, with_skips, skip_mul, device, mfma_shape)
    e = stage_errors(inputs, out, desc)
    print((B, T, dil, mfma_shape), e)
    assert e["z"] <= RTOL, e
    # |g - g64| <= half ulp_bf16(g64) + 3e-5 max|g64|, elementwise
    assert e["g_excess_over_half_ulp"] <= RTOL, e
    assert e["skips"] <= RTOL, e
    assert e["x"] <= RTOL, e


def test_residual_is_the_fp32_input_not_its_rounded_copy(device):
    """The out-conv epilogue adds the fp32 x: rebuilding x_out with bf16(x) as the residual must miss the bar."""
    inputs, out, desc = run_layer(1, 300, 3, True, 1.0, device)
    x, c, skips, ws, bs = inputs
    x_out, g_out = out[0].double(), out[3].double()
    w_o, s_o, b_o = ws[6], ws[7], bs[2]
    conv = F.conv1d(g_out, _bf16r(w_o * s_o.view(-1, 1, 1)).double(), b_o.double())
    right = (conv + x.double()) * desc.out_mul
    wrong = (conv + _bf16r(x).double()) * desc.out_mul
    assert _rel(x_out, right) <= RTOL < _rel(x_out, wrong)


@pytest.mark.parametrize("mfma_shape", [32, 16])
def test_two_launches_are_bit_identical(mfma_shape, device):
    a = run_layer(2, 1500, 8, True, 1.0, device, mfma_shape)[1]
    b = run_layer(2, 1500, 8, True, 1.0, device, mfma_shape)[1]
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_nan_input_stays_nan_where_it_reaches(device):
    """Round-to-nearest-even keeps NaN a NaN: a NaN in x reaches the three taps' columns of z and stays there."""
    B, T, dil = 1, 200, 2
    x, c, skips, ws, bs = _inputs(B, T, dil, False)
    x[0, 5, 100] = float("nan")
    desc = ops.make_wavenet_desc(B, T, dil, out_mul=math.sqrt(0.5))
    d = lambda t: None if t is None else t.to(device).contiguous()  # noqa: E731
    img = ops.wavenet_bf16_pack_weights(desc, *[d(t) for t in ws])
    _, _, z, _ = ops.wavenet_bf16_layer_forward(desc, d(x), d(c), None, img, *[d(t) for t in bs], save=True)
    z = z.cpu()
    nan_cols = torch.isnan(z[0]).any(0).nonzero().flatten().tolist()
    assert nan_cols == [100 - dil, 100, 100 + dil]
