"""GPU: the bf16-operand convolution kernel (csrc/conv1d_bf16.hip) per layer, tight.

Inputs and weights are drawn and then rounded to bf16-representable fp32 values BEFORE the call (with a pre-activation:
the activation is computed in fp32 and the ACTIVATED input is rounded, which is what the kernel rounds).  The product of
two bf16 values is exact in fp32, so the GPU result can differ from a float64 convolution of the same rounded operands
only by fp32 accumulation order: the bar is the project's existing fp32 per-layer bar (RTOL of test_conv_ops_gpu.py),
not a new number.
"""
import pytest
import torch
import torch.nn.functional as F

from parallelwavegan_amd import ops
from tests.util import poison_empty, poison_lds

pytestmark = pytest.mark.gpu

RTOL = 3e-5  # == tests/test_conv_ops_gpu.py::RTOL (relative to the largest reference magnitude)


def _bf16r(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _act(x, kind, slope):
    if kind == "leaky_relu":
        return F.leaky_relu(x, slope)
    if kind == "relu":
        return F.relu(x)
    if kind == "tanh":
        return torch.tanh(x)
    return x


def case(B, Cin, Cout, T, K, dil=1, stride=1, transposed=False, pre=None, slope=0.1, bias=True, add1=False, add2=False,
         mul=1.0, div=1.0, post=None, post_slope=0.0):
    return dict(B=B, Cin=Cin, Cout=Cout, T=T, K=K, dil=dil, stride=stride, transposed=transposed, pre=pre, slope=slope,
                bias=bias, add1=add1, add2=add2, mul=mul, div=div, post=post, post_slope=post_slope)


def _id(c):
    s = f"{'T' if c['transposed'] else 'C'}{c['Cin']}-{c['Cout']}k{c['K']}d{c['dil']}s{c['stride']}B{c['B']}T{c['T']}"
    for k in ("pre", "post"):
        if c[k]:
            s += f"-{k}{c[k]}"
    for k in ("add1", "add2"):
        if c[k]:
            s += "-" + k
    if not c["bias"]:
        s += "-nobias"
    if c["mul"] != 1.0:
        s += "-mul"
    if c["div"] != 1.0:
        s += "-div"
    return s


# every distinct problem of HiFi-GAN V1 (tools/bench_conv.py's set, all three dilations), at test lengths
V1 = [case(2, 80, 512, 200, 7)]
_ch, _T = 512, 40
for _s, _k in zip((8, 8, 2, 2), (16, 16, 4, 4)):
    V1.append(case(2, _ch, _ch // 2, _T, _k, stride=_s, transposed=True, pre="leaky_relu"))
    _ch //= 2
    _T = min(_T * _s, 640)
    for _ks in (3, 7, 11):
        for _d in (1, 3, 5):
            # first convolution of a unit: LeakyReLU in front, LeakyReLU behind (the residual block's inference form)
            V1.append(case(2, _ch, _ch, _T + 3, _ks, dil=_d, pre="leaky_relu", post="leaky_relu", post_slope=0.1))
        # second convolution of the last unit of the last block: residual, MRF running sum and mean
        V1.append(case(2, _ch, _ch, _T + 3, _ks, add1=True, add2=True, div=3.0))
V1.append(case(2, 32, 1, 1000, 7, pre="leaky_relu", slope=0.01, post="tanh"))

RAGGED = [
    case(1, 64, 64, 1, 3, pre="leaky_relu"),                     # T = 1
    case(1, 64, 64, 7, 7, dil=3, pre="leaky_relu", add1=True),   # T = 7
    case(3, 128, 128, 389, 11, dil=5, pre="leaky_relu"),         # batch 3, T a multiple of no tile
    case(3, 32, 32, 517, 3, dil=2, add1=True),
    case(1, 80, 512, 1, 7),
    case(2, 48, 40, 131, 5, dil=2, pre="relu"),                  # channels a multiple of neither 32 nor the row tile
    case(2, 32, 1, 7, 7, pre="leaky_relu", slope=0.01, post="tanh"),
    case(1, 512, 256, 1, 16, stride=8, transposed=True, pre="leaky_relu"),
    case(3, 64, 32, 7, 4, stride=2, transposed=True, pre="leaky_relu"),
    case(2, 128, 64, 45, 10, stride=5, transposed=True, pre="leaky_relu"),   # LibriTTS scales: odd stride,
    case(2, 64, 32, 77, 6, stride=3, transposed=True, pre="leaky_relu"),     # output_padding = 1
    case(2, 96, 48, 33, 8, stride=4, transposed=True),
    # lengths that are multiples of 4 take the 16-B staging path; its window starts up to 3 columns early
    case(2, 256, 256, 324, 11, dil=5, pre="leaky_relu"),
    case(2, 128, 128, 644, 3, dil=3, pre="leaky_relu", add1=True),
    case(3, 32, 32, 1028, 7, dil=5, add1=True, add2=True, div=3.0),
    case(2, 64, 64, 4, 11, dil=5, pre="leaky_relu"),
    case(1, 32, 32, 8, 3, pre="leaky_relu"),
    case(2, 256, 128, 44, 16, stride=8, transposed=True, pre="leaky_relu"),
    # launches of fewer than 256 workgroups run on half-size tiles (all of the above): these reach the full-size tiles,
    # on the 4-byte staging path (odd lengths) and on the 16-byte one
    case(3, 128, 128, 11003, 3, dil=3, pre="leaky_relu", add1=True),
    case(2, 64, 64, 16401, 7, dil=3, pre="leaky_relu"),
    case(1, 32, 32, 65541, 3, dil=5, add1=True),
    case(4, 64, 32, 8201, 4, stride=2, transposed=True, pre="leaky_relu"),
    case(4, 256, 256, 4100, 11, dil=5, pre="leaky_relu"),
]

# every fused term on and off
_F = dict(B=2, Cin=64, Cout=64, T=300, K=7, dil=3)
FUSED = [
    case(**_F, bias=False),
    case(**_F, pre="leaky_relu"),
    case(**_F, pre="relu"),
    case(**_F, add1=True),
    case(**_F, add2=True),
    case(**_F, mul=0.37),
    case(**_F, div=3.0),
    case(**_F, post="tanh"),
    case(**_F, post="leaky_relu", post_slope=0.2),
    case(**_F, post="relu"),
    case(**_F, pre="leaky_relu", add1=True, add2=True, mul=1.7, div=3.0, post="tanh"),
    case(2, 128, 64, 50, 4, stride=2, transposed=True, pre="leaky_relu", bias=False, add1=True, add2=True, mul=0.5, div=3.0,
         post="tanh"),
]

ALL = V1 + RAGGED + FUSED


def run_case(c, device, mfma_shape=None, return_error=False):
    g = torch.Generator().manual_seed(c["B"] * 7919 + c["Cin"] * 31 + c["K"] * 7 + c["T"])
    B, Cin, Cout, T, K, s, d = c["B"], c["Cin"], c["Cout"], c["T"], c["K"], c["stride"], c["dil"]
    x = _bf16r(torch.randn(B, Cin, T, generator=g))
    if c["transposed"]:
        w = _bf16r(torch.randn(Cin, Cout, K, generator=g) / (Cin * 2) ** 0.5)
        pad, opad = s // 2 + s % 2, s % 2
        t_out = ops.conv_transpose_out_length(T, K, s, pad, opad)
    else:
        w = _bf16r(torch.randn(Cout, Cin, K, generator=g) / (Cin * K) ** 0.5)
        pad = (K - 1) // 2 * d
        t_out = T
    # operands as the kernel sees them: pre-activation in fp32, then rounded to bf16
    xa = _bf16r(_act(x, c["pre"], c["slope"]))
    bias = torch.randn(Cout, generator=g) if c["bias"] else None
    add1 = torch.randn(B, Cout, t_out, generator=g) if c["add1"] else None
    add2 = torch.randn(B, Cout, t_out, generator=g) if c["add2"] else None
    if c["transposed"]:
        ref = F.conv_transpose1d(xa.double(), w.double(), None, stride=s, padding=pad, output_padding=opad)
    else:
        ref = F.conv1d(xa.double(), w.double(), None, padding=pad, dilation=d)
    assert ref.shape[-1] == t_out
    if bias is not None:
        ref = ref + bias.double()[None, :, None]
    for a in (add1, add2):
        if a is not None:
            ref = ref + a.double()
    ref = _act(ref * c["mul"] / c["div"], c["post"], c["post_slope"])

    desc = ops.make_conv_desc(B, Cin, Cout, T, t_out, K, stride=s, dilation=d, pad_left=pad, transposed=c["transposed"],
                              pre_act=c["pre"], pre_slope=c["slope"] if c["pre"] else 0.0, post_act=c["post"],
                              post_slope=c["post_slope"], out_mul=c["mul"], out_div=c["div"])
    assert ops.conv1d_bf16_supported(desc)
    dv = lambda t: None if t is None else t.to(device).contiguous()  # noqa: E731
    wp = ops.pack_weight_bf16(desc, dv(w))
    y = ops.conv1d_forward_bf16(desc, dv(x), wp, dv(bias), dv(add1), dv(add2), mfma_shape=mfma_shape)
    torch.cuda.synchronize()
    y = y.cpu().double()
    assert y.shape == ref.shape
    assert torch.isfinite(y).all(), "non-finite output"
    scale = ref.abs().max().item() + 1e-12
    err = (y - ref).abs().max().item() / scale
    print(f"{_id(c)} shape={mfma_shape}: rel-to-max error {err:.3e}")
    assert err <= RTOL, f"{_id(c)}: rel-to-max error {err:.3e} > {RTOL}"
    return (y, err) if return_error else y


@pytest.mark.parametrize("c", ALL, ids=_id)
def test_bf16_conv_matches_float64_of_rounded_operands(c, device):
    run_case(c, device)


@pytest.mark.parametrize("mfma_shape", [32, 16])
@pytest.mark.parametrize("c", V1[::5] + RAGGED + FUSED[-2:], ids=_id)
def test_both_mfma_shapes(c, mfma_shape, device):
    run_case(c, device, mfma_shape)


def test_all_cases_under_lds_and_allocation_poison(device):
    """Stale LDS (NaN-filled before every launch) and NaN-filled fresh allocations must not reach any result."""
    with poison_lds(), poison_empty():
        for c in ALL:
            run_case(c, device)
        for c in RAGGED:
            run_case(c, device, 16)


def test_weight_norm_scale_is_folded_by_the_packer(device):
    """``scale`` contract of pwg_conv1d_pack_weight: the image of (v, scale) equals the image of v * scale."""
    g = torch.Generator().manual_seed(11)
    for transposed in (False, True):
        shape = (64, 48, 4) if transposed else (48, 64, 5)
        v = torch.randn(shape, generator=g).to(device)
        scale = (torch.rand(shape[0], generator=g) + 0.5).to(device)
        desc = (ops.make_conv_desc(1, 64, 48, 16, 32, 4, stride=2, pad_left=1, transposed=True) if transposed
                else ops.make_conv_desc(1, 64, 48, 16, 16, 5, pad_left=2))
        a = ops.pack_weight_bf16(desc, v, scale)
        b = ops.pack_weight_bf16(desc, (v * scale.reshape(-1, 1, 1)).contiguous())
        assert torch.equal(a, b)


def test_bf16_conv_is_deterministic_and_rounds_like_torch(device):
    """Two launches are bit-identical, and un-rounded operands are rounded to nearest-even exactly as
    ``.to(torch.bfloat16)`` does (the CPU emulation's definition): the result equals the launch on pre-rounded operands
    bit for bit."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 64, 333, generator=g).to(device)
    w = (torch.randn(64, 64, 7, generator=g) / 21.0).to(device)
    desc = ops.make_conv_desc(2, 64, 64, 333, 333, 7, dilation=3, pad_left=9)
    y1 = ops.conv1d_forward_bf16(desc, x, ops.pack_weight_bf16(desc, w))
    y2 = ops.conv1d_forward_bf16(desc, x, ops.pack_weight_bf16(desc, w))
    y3 = ops.conv1d_forward_bf16(desc, _bf16r(x), ops.pack_weight_bf16(desc, _bf16r(w)))
    assert torch.equal(y1, y2)
    assert torch.equal(y1, y3)
    nan = x.clone()
    nan[0, 3, 100] = float("nan")  # the cast keeps NaN a NaN
    assert torch.isnan(ops.conv1d_forward_bf16(desc, nan, ops.pack_weight_bf16(desc, w))[0, :, 100]).all()


def test_unsupported_descriptor_is_an_error_not_a_fallback(device):
    desc = ops.make_conv_desc(1, 16, 16, 32, 32, 3, pad_left=1, groups=4)
    assert not ops.conv1d_bf16_supported(desc)
    with pytest.raises(RuntimeError):
        ops.pack_weight_bf16(desc, torch.zeros(16, 4, 3, device=device))
