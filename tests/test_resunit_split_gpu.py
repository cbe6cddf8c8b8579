"""GPU: the split-operand residual unit (csrc/resunit_split.hip, ``ops.resunit_forward_split``).

The oracle is the chain the kernel is defined by: two ``ops.conv1d_forward_split`` launches at the same
MFMA shape -- conv1 with ``pre_act = post_act = leaky`` and bias b1, conv2 with bias b2, ``add1 = x``, add2 and out_div --
and the comparison is ``torch.equal``.  Every case also runs against a float64 unit of the same fp32 operands (the
pre-activation of x applied in fp32, as tests/test_conv_split_gpu.py does), error relative to the largest output, gate
3e-5 (the project's fp32 bar), and prints ``split_error / fp32_unit_error`` (``ops.resunit_forward`` on the same inputs),
whose median over all cases must stay below 2, the bar of DESIGN.md s9.1.

Shapes: C = 32 and 64; (k, d) = (3, 1), (3, 5), (7, 3), (11, 1), (11, 5); the pair and the single-convolution form;
(batch, T) = (2, 100): shorter than one tile, halo beyond both ends; (3, 1000): a few tiles, the last one ragged;
(2, 4148): many tiles.  Each launch runs under poisoned LDS and a poisoned output, into a guarded view, twice."""
import functools
import itertools
import statistics

import pytest
import torch
import torch.nn.functional as F

from parallelwavegan_amd import _lib, ops
from tests.test_conv_split_gpu import Guarded
from tests.util import poison_empty, poison_lds

pytestmark = pytest.mark.gpu

RTOL = 3e-5
RATIO_BAR = 2.0
SLOPE = 0.1

KD = [(3, 1), (3, 5), (7, 3), (11, 1), (11, 5)]
BT = [(2, 100), (3, 1000), (2, 4148)]
VARIANTS = {
    "plain": dict(bias=False, add2=False, out_div=1.0),
    "all": dict(bias=True, add2=True, out_div=3.0),
    "bias": dict(bias=True, add2=False, out_div=1.0),
    "add2": dict(bias=False, add2=True, out_div=1.0),
    "div3": dict(bias=False, add2=False, out_div=3.0),
}

# (C, k, d, pair, batch, T, variant, kind)
CASES = [(c, k, d, pair, b, t, v, "randn")
         for c, (k, d), pair, (b, t), v in itertools.product((32, 64), KD, (True, False), BT, ("plain", "all"))]
# each epilogue term alone, at a few tiles with a ragged last one
CASES += [(32, 7, 3, True, 3, 1000, v, "randn") for v in ("bias", "add2", "div3")]
CASES += [(64, 3, 5, False, 3, 1000, v, "randn") for v in ("bias", "add2", "div3")]
# the input kinds of tests/test_conv_split_gpu.py
CASES += [(64, 7, 3, True, 3, 1000, "all", "wide"), (32, 11, 5, True, 3, 1000, "plain", "wide"),
          (64, 11, 5, True, 3, 1000, "plain", "cancel"), (32, 7, 3, True, 3, 1000, "all", "cancel")]
IDS = ["c%d_k%d_d%d_%s_b%d_t%d-%s-%s" % (c, k, d, "pair" if p else "single", b, t, v, kind)
       for c, k, d, p, b, t, v, kind in CASES]


@functools.lru_cache(maxsize=None)
def _inputs(c, k, b, t, kind):
    """CPU float32 inputs, shared (read-only) by every case of this size."""
    g = torch.Generator().manual_seed(c * 100003 + k * 1009 + b * 101 + t + len(kind))
    x = torch.randn(b, c, t, generator=g)
    w1 = torch.randn(c, c, k, generator=g) / (c * k) ** 0.5
    w2 = torch.randn(c, c, k, generator=g) / (c * k) ** 0.5
    if kind == "wide":  # channel magnitudes 2^-20 .. 2^20
        e = torch.linspace(-20, 20, c)[torch.randperm(c, generator=g)]
        x = x * torch.exp2(e.round()).view(1, -1, 1)
    if kind == "cancel":  # w and -w on paired channels of near-equal inputs
        u = torch.rand(b, c // 2, t, generator=g) * 2 - 1
        x[:, 1::2] = x[:, 0::2] * (1 + u / 16)
        w1[:, 1::2] = -w1[:, 0::2]
    return dict(x=x, w1=w1, w2=w2, b1=torch.randn(c, generator=g), b2=torch.randn(c, generator=g),
                add2=torch.randn(b, c, t, generator=g))


def _conv64(x, w, dil):
    """The bare 'same' convolution in float64 as k matrix products over shifted views."""
    k, t = w.shape[2], x.shape[2]
    pad = (k - 1) // 2 * dil
    xp = F.pad(x, (pad, pad))
    y = torch.zeros(x.shape[0], w.shape[0], t, dtype=torch.float64)
    for tap in range(k):
        y += torch.matmul(w[:, :, tap], xp[:, :, tap * dil:tap * dil + t])
    return y


@functools.lru_cache(maxsize=None)
def _ref(c, k, d, pair, b, t, variant, kind):
    """The unit in float64 from the fp32 operands; lrelu(x) is formed in fp32, as the kernels define it."""
    i, v = _inputs(c, k, b, t, kind), VARIANTS[variant]
    h = _conv64(F.leaky_relu(i["x"], SLOPE).double(), i["w1"].double(), d)
    if v["bias"]:
        h = h + i["b1"].double().view(1, -1, 1)
    if pair:
        h = _conv64(F.leaky_relu(h, SLOPE), i["w2"].double(), 1)
        if v["bias"]:
            h = h + i["b2"].double().view(1, -1, 1)
    y = h + i["x"].double()
    if v["add2"]:
        y = y + i["add2"].double()
    return y / v["out_div"]


def _chain(c, k, d, pair, b, t, out_div, x, i1, i2, b1, b2, add2, shape):
    """The defining chain of general split launches."""
    pad = (k - 1) // 2
    if not pair:
        d1 = ops.make_conv_desc(b, c, c, t, t, k, 1, d, pad * d, pre_act="leaky_relu", pre_slope=SLOPE, out_div=out_div)
        return ops.conv1d_forward_split(d1, x, i1, b1, x, add2, mfma_shape=shape)
    d1 = ops.make_conv_desc(b, c, c, t, t, k, 1, d, pad * d, pre_act="leaky_relu", pre_slope=SLOPE,
                            post_act="leaky_relu", post_slope=SLOPE)
    d2 = ops.make_conv_desc(b, c, c, t, t, k, 1, 1, pad, out_div=out_div)
    h = ops.conv1d_forward_split(d1, x, i1, b1, mfma_shape=shape)
    return ops.conv1d_forward_split(d2, h, i2, b2, x, add2, mfma_shape=shape)


@functools.lru_cache(maxsize=None)
def _run(c, k, d, pair, b, t, variant, kind):
    device = torch.device("cuda:0")
    i, v = _inputs(c, k, b, t, kind), VARIANTS[variant]
    x, w1, w2 = i["x"].to(device), i["w1"].to(device), i["w2"].to(device)
    b1, b2 = (i[n].to(device) if v["bias"] else None for n in ("b1", "b2"))
    add2 = i["add2"].to(device) if v["add2"] else None
    ref = _ref(c, k, d, pair, b, t, variant, kind).to(device)
    scale = float(ref.abs().max()) + 1e-300
    desc = ops.make_resunit_desc(b, c, t, k, d, pair, SLOPE, SLOPE, v["out_div"])
    assert ops.resunit_split_supported(desc)
    what = f"C{c} k{k} d{d} pair{pair} B{b} T{t} {variant} {kind}"

    def err(y):
        return float((y.double() - ref).abs().max()) / scale

    def unit(shape):
        gd = Guarded(tuple(x.shape), device)
        ops.resunit_forward_split(desc, x, i1, b1, i2 if pair else None, b2 if pair else None, add2, out=gd.out,
                                  mfma_shape=shape)
        return gd.check(f"{what} mfma {shape}")

    wdesc = ops.make_conv_desc(1, c, c, 64, 64, k, pad_left=(k - 1) // 2)
    with poison_lds(), poison_empty():
        i1, i2 = ops.pack_weight_split(wdesc, w1), ops.pack_weight_split(wdesc, w2)
        y16, again, y32 = unit(16), unit(16), unit(32)
        default = ops.resunit_forward_split(desc, x, i1, b1, i2 if pair else None, b2 if pair else None, add2)
        c16 = _chain(c, k, d, pair, b, t, v["out_div"], x, i1, i2, b1, b2, add2, 16)
        c32 = _chain(c, k, d, pair, b, t, v["out_div"], x, i1, i2, b1, b2, add2, 32)
        y_fp32 = ops.resunit_forward(desc, x, ops.resunit_pack_weight(w1), b1,
                                     ops.resunit_pack_weight(w2) if pair else None, b2 if pair else None, add2)
    return dict(err=err(y16), err32=err(y32), err_fp32=err(y_fp32), repeat=torch.equal(y16, again),
                default=torch.equal(default, y16), chain16=torch.equal(y16, c16), chain32=torch.equal(y32, c32),
                diff16=float((y16 - c16).abs().max()), diff32=float((y32 - c32).abs().max()))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_unit(case, device):
    r = _run(*case)
    ratio = r["err"] / max(r["err_fp32"], 1e-300)
    print(f"rel-to-max error: split unit {r['err']:.3e} (32x32x16: {r['err32']:.3e})  fp32 unit {r['err_fp32']:.3e}  "
          f"ratio {ratio:.2f}  |unit - chain| {r['diff16']:.3e} / {r['diff32']:.3e}")
    assert r["chain16"], f"16x16x32: differs from the chained split launches by {r['diff16']:.3e}"
    assert r["chain32"], f"32x32x16: differs from the chained split launches by {r['diff32']:.3e}"
    assert r["repeat"], "two launches on the same inputs differ"
    assert r["default"], "the default launch is not the 16x16x32 one"
    assert r["err"] <= RTOL, f"rel-to-max error {r['err']:.3e}"
    assert r["err32"] <= RTOL, f"32x32x16: rel-to-max error {r['err32']:.3e}"


def test_median_error_ratio(device):
    """Median over all cases of split_unit_error / fp32_unit_error < 2."""
    ratios = []
    for case in CASES:
        r = _run(*case)
        ratios.append(r["err"] / max(r["err_fp32"], 1e-300))
    print("ratios: " + " ".join(f"{q:.2f}" for q in ratios) + f"  median {statistics.median(ratios):.3f}")
    assert statistics.median(ratios) < RATIO_BAR


def test_weight_norm_scale_folds_into_the_image(device):
    torch.manual_seed(5)
    c, k, d, t = 32, 7, 3, 2048
    x = torch.randn(2, c, t)
    v = torch.randn(c, c, k)
    g = torch.rand(c) + 0.5
    scale = g / v.reshape(c, -1).norm(dim=1)
    w = v * scale[:, None, None]
    desc = ops.make_resunit_desc(2, c, t, k, d, False, SLOPE, SLOPE, 1.0)
    wdesc = ops.make_conv_desc(1, c, c, 64, 64, k, pad_left=(k - 1) // 2)
    y = ops.resunit_forward_split(desc, x.to(device), ops.pack_weight_split(wdesc, v.to(device), scale.to(device)), None)
    ref = _conv64(F.leaky_relu(x, SLOPE).double(), w.double(), d) + x.double()
    assert float((y.cpu().double() - ref).abs().max() / ref.abs().max()) <= RTOL


def test_refused_geometries_launch_nothing(device):
    """Every refusal is a host decision with a message: the output keeps its sentinel."""
    c, k, t = 32, 3, 64
    x = torch.randn(1, c, t, device=device)

    def image(kernel):
        wdesc = ops.make_conv_desc(1, c, c, 64, 64, kernel, pad_left=(kernel - 1) // 2)
        return ops.pack_weight_split(wdesc, torch.randn(c, c, kernel, device=device))

    img = image(k)
    ok = ops.make_resunit_desc(1, c, t, k, 1, True)

    def refused(desc, xx, w1, w2, out, match, **kw):
        before = out.clone()
        with ops.profile() as prof:
            with pytest.raises(RuntimeError, match=match):
                ops.resunit_forward_split(desc, xx, w1, None, w2, None, None, out=out, **kw)
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), before.view(torch.int32))
        assert not any("resunit_split_kernel" in name for name in prof.results)

    out = torch.full_like(x, float("nan"))
    # kernel size, T % 4, LDS window
    img4 = image(4)
    refused(ops.make_resunit_desc(1, c, t, 4, 1, True), x, img4, img4, out, "odd")
    x66 = torch.randn(1, c, 66, device=device)
    refused(ops.make_resunit_desc(1, c, 66, k, 1, True), x66, img, img, torch.full_like(x66, float("nan")), "multiple of 4")
    refused(ops.make_resunit_desc(1, c, t, k, 60, True), x, img, img, out, "LDS")
    # y aliases x, the second image is missing, a misaligned view, an unknown MFMA shape
    refused(ok, x, img, img, x, "alias")
    refused(ok, x, img, None, out, "w2_packed")
    buf = torch.full((c * t + 4,), float("nan"), device=device)
    refused(ok, x, img, img, buf[1:1 + c * t].view(1, c, t), "aligned")
    refused(ok, x, img, img, out, "mfma_shape", mfma_shape=8)
    assert not ops.resunit_split_supported(ops.make_resunit_desc(1, 128, t, k, 1, True))
    assert "channels" in _lib.lib().pwg_last_error().decode()
