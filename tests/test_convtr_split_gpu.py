"""GPU: the split-operand transposed convolution (csrc/conv1d_split.hip, ``convtr1d_split_mfma_kernel``,
``ops.conv1d_forward_split_transposed``) against ``F.conv_transpose1d`` in float64 of the same fp32
operands on the CPU (the pre-activation applied in fp32 first), error relative to the largest reference magnitude, gate
RTOL = 3e-5 (the project's op-level bar, tests/test_conv_split_gpu.py).

Every launch writes into a guarded, NaN-poisoned view under poisoned LDS, is repeated (run-to-run bits), runs at both MFMA
shapes and on full-size and half-size tiles (same bits).  Every case also runs the fp32 kernel (``ops.conv1d_forward``)
on the same inputs: ``split_error / fp32_error`` is printed per case and its median over all cases must stay below 2.
Wherever the stride-1 split kernel can express the layer's twin (k = 2, pad_left = 1, rows co * s + phase), the two must
agree bit for bit after the phase interleave."""
import functools
import statistics

import pytest
import torch
import torch.nn.functional as F

from parallelwavegan_amd import ops
from tests import test_conv_split_gpu as conv_split
from tests.test_conv_split_gpu import RATIO_BAR, RTOL, Guarded, _act
from tests.util import poison_empty, poison_lds

pytestmark = pytest.mark.gpu

# The variants of tests/test_conv_split_gpu.py, and "all" without the tanh for the `wide` inputs: their outputs reach
# 2^20, so an fp32 accumulation error of 2^-24 of the largest product is ~0.06 in absolute terms, and tanh of an output
# that happens to fall near zero carries it over undamped while the reference's largest magnitude is 1 -- the case would
# measure where the outputs fall, not the kernel (any fp32 kernel misses 3e-5 on it; measured on the fp32 kernel: 1.1e-4).
VARIANTS = dict(conv_split.VARIANTS)
VARIANTS["all_linear"] = dict(VARIANTS["all"], post_act=None)


def _variant(name):
    v = dict(bias=False, add1=False, add2=False, out_div=1.0, pre_act=None, pre_slope=0.0, post_act=None)
    v.update(VARIANTS[name])
    return v


SHAPES = {
    # channel tail; m = 72 padded to the 128-row tile; 4-byte staging; 16-byte epilogue
    "c40_co9_s8_t37": dict(B=2, cin=40, cout=9, s=8, T=37),
    # 64-row tile; 16-byte staging; the odd-start pairs of s = 2
    "c64_co24_s2_t512": dict(B=1, cin=64, cout=24, s=2, T=512),
    # 32-row tile; one column tile whose q - 1 tap lies in front of the input
    "c40_co16_s2_t128": dict(B=1, cin=40, cout=16, s=2, T=128),
    # m = 128 exactly; a second column tile of a few columns, the last q masked above phase 3
    "c64_co16_s8_t130": dict(B=2, cin=64, cout=16, s=8, T=130),
    # t_out = 202: the 4-byte epilogue
    "c64_co24_s2_t101": dict(B=2, cin=64, cout=24, s=2, T=101),
    # odd stride (MB-MelGAN's k = 10, s = 5, padding 3, output_padding 1): four consecutive rows straddle channels
    "c32_co8_s5_t64": dict(B=1, cin=32, cout=8, s=5, T=64),
    # 33 column tiles x 2 row blocks x 4 items: full-size tiles by the small-grid rule, half-size when forced
    "c64_co32_s8_t4096": dict(B=4, cin=64, cout=32, s=8, T=4096),
}
FIRST = "c40_co9_s8_t37"
CASES = ([(FIRST, v, "randn") for v in conv_split.VARIANTS]
         + [(s, v, "randn") for s in SHAPES if s != FIRST for v in ("plain", "all")]
         + [(FIRST, "plain", "wide"), ("c64_co24_s2_t512", "all_linear", "wide"),
            (FIRST, "plain", "cancel"), ("c64_co24_s2_t512", "plain", "cancel")])
IDS = [f"{s}-{v}-{kind}" for s, v, kind in CASES]


def _geom(s):
    """kernel, padding, output_padding, t_out of a shape: the upsampling layers' k = 2s, padding s // 2 + s % 2."""
    st = s["s"]
    k, p, op = 2 * st, st // 2 + st % 2, st % 2
    return k, p, op, ops.conv_transpose_out_length(s["T"], k, st, p, op)


@functools.lru_cache(maxsize=None)
def _inputs(shape, kind):
    """CPU float32 inputs, shared (read-only) by every test of (shape, kind)."""
    s = SHAPES[shape]
    k, _, _, t_out = _geom(s)
    g = torch.Generator().manual_seed(sum(map(ord, shape + kind)) * 131 + s["cin"])
    x = torch.randn(s["B"], s["cin"], s["T"], generator=g)
    w = torch.randn(s["cin"], s["cout"], k, generator=g) / (s["cin"] * 2) ** 0.5
    if kind == "wide":
        e = torch.linspace(-20, 20, s["cin"])[torch.randperm(s["cin"], generator=g)]
        x = x * torch.exp2(e.round()).view(1, -1, 1)
    if kind == "cancel":  # as tests/test_conv_split_gpu.py: near-equal inputs on paired channels under w and -w
        u = torch.rand(s["B"], s["cin"] // 2, s["T"], generator=g) * 2 - 1
        x[:, 1::2] = x[:, 0::2] * (1 + u / 16)
        w[1::2] = -w[0::2]
    bias = torch.randn(s["cout"], generator=g)
    add1 = torch.randn(s["B"], s["cout"], t_out, generator=g)
    add2 = torch.randn(s["B"], s["cout"], t_out, generator=g)
    return dict(x=x, w=w, bias=bias, add1=add1, add2=add2)


@functools.lru_cache(maxsize=None)
def _convtr_ref(shape, kind, pre_act, pre_slope):
    s, t = SHAPES[shape], _inputs(shape, kind)
    _, p, op, _ = _geom(s)
    return F.conv_transpose1d(_act(t["x"], pre_act, pre_slope).double(), t["w"].double(), stride=s["s"], padding=p,
                              output_padding=op)


@functools.lru_cache(maxsize=None)
def _ref(shape, variant, kind):
    t, v = _inputs(shape, kind), _variant(variant)
    y = _convtr_ref(shape, kind, v["pre_act"], v["pre_slope"])
    if v["bias"]:
        y = y + t["bias"].double().view(1, -1, 1)
    if v["add1"]:
        y = y + t["add1"].double()
    if v["add2"]:
        y = y + t["add2"].double()
    return _act(y / v["out_div"], v["post_act"])


def _desc(shape, variant):
    s, v = SHAPES[shape], _variant(variant)
    k, p, _, t_out = _geom(s)
    return ops.make_conv_desc(s["B"], s["cin"], s["cout"], s["T"], t_out, k, s["s"], 1, p, transposed=True,
                              pre_act=v["pre_act"], pre_slope=v["pre_slope"], post_act=v["post_act"], out_div=v["out_div"])


@functools.lru_cache(maxsize=None)
def _run(shape, variant, kind):
    """One case on the GPU, run once and shared."""
    device = torch.device("cuda:0")
    v, t = _variant(variant), _inputs(shape, kind)
    desc = _desc(shape, variant)
    assert ops.convtr1d_split_supported(desc)
    x, w = t["x"].to(device), t["w"].to(device)
    bias, add1, add2 = (t[n].to(device) if v[n] else None for n in ("bias", "add1", "add2"))
    ref = _ref(shape, variant, kind).to(device)
    scale = float(ref.abs().max()) + 1e-300
    what = f"{shape} {variant} {kind}"

    def err(y):
        return float((y.double() - ref).abs().max()) / scale

    def split(**cfg):
        gd = Guarded(tuple(ref.shape), device)
        ops.conv1d_forward_split_transposed(desc, x, ws, bias, add1, add2, out=gd.out, **cfg)
        return gd.check(f"{what} {cfg}")

    with poison_lds(), poison_empty():
        ws = ops.pack_weight_split_transposed(desc, w)
        y = split()
        again = split()
        full, half = split(tile_mode=1), split(tile_mode=2)
        y32, half32 = split(mfma_shape=32), split(mfma_shape=32, tile_mode=2)
        y_fp32 = ops.conv1d_forward(desc, x, ops.pack_weight(desc, w), bias, add1, add2)
    return dict(err=err(y), err32=err(y32), err_fp32=err(y_fp32), repeat=torch.equal(y, again),
                tiles=torch.equal(full, half) and torch.equal(y, full) and torch.equal(y32, half32), y=y, y32=y32)


@pytest.mark.parametrize("shape,variant,kind", CASES, ids=IDS)
def test_split_transposed_forward(shape, variant, kind, device):
    r = _run(shape, variant, kind)
    ratio = r["err"] / max(r["err_fp32"], 1e-300)
    print(f"rel-to-max error: split {r['err']:.3e} (32x32x16: {r['err32']:.3e})  fp32 kernel {r['err_fp32']:.3e}  "
          f"ratio {ratio:.2f}")
    assert r["err"] <= RTOL, f"rel-to-max error {r['err']:.3e}"
    assert r["err32"] <= RTOL, f"32x32x16: rel-to-max error {r['err32']:.3e}"
    assert r["repeat"], "two launches on the same inputs differ"
    assert r["tiles"], "full-size and half-size tiles differ"


def test_median_error_ratio(device):
    """Median over all cases of split_error / fp32_kernel_error < 2 (the rule of DESIGN.md s9.1)."""
    ratios = []
    for case in CASES:
        r = _run(*case)
        ratios.append(r["err"] / max(r["err_fp32"], 1e-300))
    print("ratios: " + " ".join(f"{q:.2f}" for q in ratios) + f"  median {statistics.median(ratios):.3f}")
    assert statistics.median(ratios) < RATIO_BAR


@pytest.mark.parametrize("variant", ["plain", "all"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_bit_identity_with_the_stride_1_twin(shape, variant, device):
    """The layer as a stride-1 convolution -- k = 2, pad_left = 1, rows co * s + phase, tap 0 = w[ci][co][phase + s],
    tap 1 = w[ci][co][phase] -- on ``ops.conv1d_forward_split``, then the phase interleave in torch: the same products
    in the same order, so the same bits, at both MFMA shapes.  (The addends of ``all`` are de-interleaved for the twin;
    samples the layer does not have read as zero there and are cut off.)"""
    s, v, t = SHAPES[shape], _variant(variant), _inputs(shape, "randn")
    st, B, cout = s["s"], s["B"], s["cout"]
    _, p, _, t_out = _geom(s)
    nq = -(-(t_out + p) // st)
    twin = ops.make_conv_desc(B, s["cin"], cout * st, s["T"], nq, 2, 1, 1, 1, pre_act=v["pre_act"],
                              pre_slope=v["pre_slope"], post_act=v["post_act"], out_div=v["out_div"])
    assert ops.conv1d_split_supported(twin)
    x, w = t["x"].to(device), t["w"].to(device)
    # (ci, co, 2, s) -> rows co * s + phase, taps (phase + s, phase)
    w2 = w.view(s["cin"], cout, 2, st).flip(2).permute(1, 3, 0, 2).reshape(cout * st, s["cin"], 2).contiguous()

    def to_twin(a):  # (B, cout, t_out) -> (B, cout * s, nq), zero where the layer has no sample
        full = torch.zeros(B, cout, nq * st, device=device)
        full[:, :, p:p + t_out] = a.to(device)
        return full.view(B, cout, nq, st).permute(0, 1, 3, 2).reshape(B, cout * st, nq).contiguous()

    bias = t["bias"].to(device).repeat_interleave(st) if v["bias"] else None
    add1 = to_twin(t["add1"]) if v["add1"] else None
    add2 = to_twin(t["add2"]) if v["add2"] else None
    r = _run(shape, variant, "randn")
    ws2 = ops.pack_weight_split(twin, w2)
    for mfma_shape, y in ((16, r["y"]), (32, r["y32"])):
        y2 = ops.conv1d_forward_split(twin, x, ws2, bias, add1, add2, mfma_shape=mfma_shape)
        inter = y2.view(B, cout, st, nq).permute(0, 1, 3, 2).reshape(B, cout, nq * st)[:, :, p:p + t_out]
        assert torch.equal(inter, y), f"{shape} {variant}: MFMA shape {mfma_shape} differs from the stride-1 twin"


def test_image_is_three_parts_of_the_bf16_transposed_image(device):
    """One layout, one owner: the hi part is the bf16 kernel's transposed image byte for byte, weight-norm scale (per
    input channel) included."""
    g = torch.Generator().manual_seed(9)
    w = torch.randn(40, 9, 16, generator=g).to(device)
    scale = (torch.rand(40, generator=g) + 0.5).to(device)
    desc = ops.make_conv_desc(1, 40, 9, 8, 64, 16, 8, 1, 4, transposed=True)
    image, parts = ops.pack_weight_bf16(desc, w, scale), ops.pack_weight_split_transposed(desc, w, scale)
    assert parts.numel() == 3 * image.numel()
    assert torch.equal(parts[:image.numel()], image)
