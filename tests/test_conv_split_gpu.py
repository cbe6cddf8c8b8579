"""GPU: the split-operand fp32 convolution (csrc/conv1d_split.hip, ``ops.conv1d_forward_split``) against a float64
convolution of the same fp32 operands on the CPU, error relative to the largest reference magnitude, gate RTOL = 3e-5
(the project's fp32 bound, tests/test_conv_cfg_matrix_gpu.py).

The shapes are the smallest that reach every path of the kernel: a channel tail inside a 32-channel chunk (Cin = 40) and
whole chunks (64); the 128- / 64- / 32-row tiles with padded rows (Cout = 72 / 48 / 24); k = 7 dilation 3 and k = 11
dilation 5; T = 203 (4-byte staging) and T = 512 (16-byte staging); T = 128 at batch 1 (one column tile whose halo lies
beyond both ends of the input); batch 2; and one launch of 256 workgroups, from which the small-grid rule keeps the
full-size tiles.  Every launch writes into a guarded view, is repeated (run-to-run bits) and is run on full-size and on
half-size tiles (same bits).  Every case also runs the fp32 MFMA kernel (``ops.conv1d_forward``) on the same inputs:
``split_error / fp32_error`` is printed per case, and its median over all cases must stay below 2 -- the bar of
DESIGN.md s9 for "one more realisation of the same rounding process" -- for the six-product, one-accumulator form."""
import functools
import math
import statistics

import pytest
import torch
import torch.nn.functional as F

from parallelwavegan_amd import ops
from tests.util import poison_empty, poison_lds

pytestmark = pytest.mark.gpu

RTOL = 3e-5
RATIO_BAR = 2.0
GUARD = 64
SENTINEL = 0x7FC5A5A5

SHAPES = {
    # channel tail, 128-row tile with padded rows, 4-byte staging, batch 2
    "c40_m72_k7_t203": dict(B=2, cin=40, cout=72, T=203, k=7, dil=3),
    # whole chunks, 64-row tile, 16-byte staging, the widest window
    "c64_m48_k11_t512": dict(B=1, cin=64, cout=48, T=512, k=11, dil=5),
    # 32-row tile, one column tile at batch 1, halo of 25 columns beyond both ends
    "c40_m24_k11_t128": dict(B=1, cin=40, cout=24, T=128, k=11, dil=5),
    "c64_m24_k7_t512": dict(B=2, cin=64, cout=24, T=512, k=7, dil=3),
    # the full-size 32 x 256 tile (three planes fit 64 KB of LDS up to a halo of 13 columns; the two above run 32 x 128)
    "c64_m24_k7d1_t515": dict(B=2, cin=64, cout=24, T=515, k=7, dil=1),
    "c64_m72_k11_t512": dict(B=2, cin=64, cout=72, T=512, k=11, dil=5),
    "c40_m48_k7_t203": dict(B=2, cin=40, cout=48, T=203, k=7, dil=3),
    # 32 column tiles x 2 row blocks x 4 items = 256 workgroups: full-size tiles by the rule, half-size when forced
    "c256_m256_k7_t4096": dict(B=4, cin=256, cout=256, T=4096, k=7, dil=1),
}

# bias, add1, add2, out_div, pre_act, post_act: each alone and all together
VARIANTS = {
    "plain": dict(),
    "bias": dict(bias=True),
    "add1": dict(add1=True),
    "add2": dict(add2=True),
    "div3": dict(out_div=3.0),
    "pre_lrelu": dict(pre_act="leaky_relu", pre_slope=0.1),
    "post_tanh": dict(post_act="tanh"),
    "all": dict(bias=True, add1=True, add2=True, out_div=3.0, pre_act="leaky_relu", pre_slope=0.1, post_act="tanh"),
}

# input kinds: "randn"; "wide": channel magnitudes 2^-20 .. 2^20; "cancel": w and -w on paired channels of near-equal inputs
CASES = ([("c40_m72_k7_t203", v, "randn") for v in VARIANTS]
         + [(s, v, "randn") for s in SHAPES if s != "c40_m72_k7_t203" for v in ("plain", "all")]
         + [("c40_m72_k7_t203", "plain", "wide"), ("c64_m48_k11_t512", "all", "wide"),
            ("c40_m72_k7_t203", "plain", "cancel"), ("c64_m48_k11_t512", "plain", "cancel")])
IDS = [f"{s}-{v}-{kind}" for s, v, kind in CASES]


def _variant(name):
    v = dict(bias=False, add1=False, add2=False, out_div=1.0, pre_act=None, pre_slope=0.0, post_act=None)
    v.update(VARIANTS[name])
    return v


@functools.lru_cache(maxsize=None)
def _inputs(shape, kind):
    """CPU float32 inputs, shared (read-only) by every test of (shape, kind)."""
    s = SHAPES[shape]
    g = torch.Generator().manual_seed(sum(map(ord, shape + kind)) * 131 + s["cin"])
    x = torch.randn(s["B"], s["cin"], s["T"], generator=g)
    w = torch.randn(s["cout"], s["cin"], s["k"], generator=g) / (s["cin"] * s["k"]) ** 0.5
    if kind == "wide":
        e = torch.linspace(-20, 20, s["cin"])[torch.randperm(s["cin"], generator=g)]
        x = x * torch.exp2(e.round()).view(1, -1, 1)
    if kind == "cancel":
        # channel 2i + 1 = channel 2i * (1 + 2^-4 u), weights w and -w: the output is ~2^-5 of the products' size, so an
        # operand error of 2^-17 (a 2-part split) shows as ~2^-12 of the output, one of 2^-25 (3 parts) as ~2^-20
        u = torch.rand(s["B"], s["cin"] // 2, s["T"], generator=g) * 2 - 1
        x[:, 1::2] = x[:, 0::2] * (1 + u / 16)
        w[:, 1::2] = -w[:, 0::2]
    bias = torch.randn(s["cout"], generator=g)
    add1 = torch.randn(s["B"], s["cout"], s["T"], generator=g)
    add2 = torch.randn(s["B"], s["cout"], s["T"], generator=g)
    return dict(x=x, w=w, bias=bias, add1=add1, add2=add2)


def _conv64(s, x, w):
    """The bare 'same' convolution in float64 as k matrix products over shifted views (x: float64, pre-activated)."""
    pad = (s["k"] - 1) // 2 * s["dil"]
    xp = F.pad(x, (pad, pad))
    y = torch.zeros(s["B"], s["cout"], s["T"], dtype=torch.float64)
    for tap in range(s["k"]):
        y += torch.matmul(w[:, :, tap], xp[:, :, tap * s["dil"]:tap * s["dil"] + s["T"]])
    return y


def _act(t, act, slope=0.0):
    if act == "leaky_relu":
        return F.leaky_relu(t, slope)
    if act == "tanh":
        return torch.tanh(t)
    return t


@functools.lru_cache(maxsize=None)
def _conv_ref(shape, kind, pre_act, pre_slope):
    t = _inputs(shape, kind)
    # (the pre-activation is applied in fp32, as the kernels define it; for leaky_relu(0.1) float64 would differ by an ulp)
    return _conv64(SHAPES[shape], _act(t["x"], pre_act, pre_slope).double(), t["w"].double())


@functools.lru_cache(maxsize=None)
def _ref(shape, variant, kind):
    t, v = _inputs(shape, kind), _variant(variant)
    y = _conv_ref(shape, kind, v["pre_act"], v["pre_slope"])
    if v["bias"]:
        y = y + t["bias"].double().view(1, -1, 1)
    if v["add1"]:
        y = y + t["add1"].double()
    if v["add2"]:
        y = y + t["add2"].double()
    return _act(y / v["out_div"], v["post_act"])


class Guarded:
    """An output view in the middle of a sentinel-filled buffer (tests/test_conv_cfg_matrix_gpu.py)."""

    def __init__(self, shape, device):
        n = math.prod(shape)
        self.buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device=device)
        self.lo, self.hi = GUARD, GUARD + n
        self.out = self.buf[self.lo:self.hi].view(torch.float32).view(shape)

    def check(self, what):
        assert bool((self.buf[:self.lo] == SENTINEL).all()), f"{what}: store below the output"
        assert bool((self.buf[self.hi:] == SENTINEL).all()), f"{what}: store past the output"
        left = int((self.buf[self.lo:self.hi] == SENTINEL).sum())
        assert left == 0, f"{what}: {left} output elements never written"
        return self.out


@functools.lru_cache(maxsize=None)
def _run(shape, variant, kind):
    """One case on the GPU, run once and shared: errors of the split kernel (default launch, both MFMA shapes) and of
    the fp32 kernel against float64, and whether repeats and tile sizes give the same bits."""
    device = torch.device("cuda:0")
    s, v, t = SHAPES[shape], _variant(variant), _inputs(shape, kind)
    pad = (s["k"] - 1) // 2 * s["dil"]
    desc = ops.make_conv_desc(s["B"], s["cin"], s["cout"], s["T"], s["T"], s["k"], 1, s["dil"], pad, pre_act=v["pre_act"],
                              pre_slope=v["pre_slope"], post_act=v["post_act"], out_div=v["out_div"])
    assert ops.conv1d_split_supported(desc)
    x, w = t["x"].to(device), t["w"].to(device)
    bias, add1, add2 = (t[n].to(device) if v[n] else None for n in ("bias", "add1", "add2"))
    ref = _ref(shape, variant, kind).to(device)
    scale = float(ref.abs().max()) + 1e-300
    oshape = tuple(ref.shape)
    what = f"{shape} {variant} {kind}"

    def err(y):
        return float((y.double() - ref).abs().max()) / scale

    def split(**cfg):
        gd = Guarded(oshape, device)
        ops.conv1d_forward_split(desc, x, ws, bias, add1, add2, out=gd.out, **cfg)
        return gd.check(f"{what} {cfg}")

    with poison_lds(), poison_empty():
        ws = ops.pack_weight_split(desc, w)
        y = split()
        again = split()
        full, half = split(tile_mode=1), split(tile_mode=2)
        y32 = split(mfma_shape=32)
        y_fp32 = ops.conv1d_forward(desc, x, ops.pack_weight(desc, w), bias, add1, add2)
    return dict(err=err(y), err32=err(y32), err_fp32=err(y_fp32), repeat=torch.equal(y, again),
                tiles=torch.equal(full, half) and torch.equal(y, full))


@pytest.mark.parametrize("shape,variant,kind", CASES, ids=IDS)
def test_split_forward(shape, variant, kind, device):
    r = _run(shape, variant, kind)
    ratio = r["err"] / max(r["err_fp32"], 1e-300)
    print(f"rel-to-max error: split {r['err']:.3e} (32x32x16: {r['err32']:.3e})  fp32 kernel {r['err_fp32']:.3e}  "
          f"ratio {ratio:.2f}")
    assert r["err"] <= RTOL, f"rel-to-max error {r['err']:.3e}"
    assert r["err32"] <= RTOL, f"32x32x16: rel-to-max error {r['err32']:.3e}"
    assert r["repeat"], "two launches on the same inputs differ"
    assert r["tiles"], "full-size and half-size tiles differ"


def test_median_error_ratio(device):
    """Median over all cases of split_error / fp32_kernel_error < 2 (six products, one accumulator set)."""
    ratios = []
    for case in CASES:
        r = _run(*case)
        ratios.append(r["err"] / max(r["err_fp32"], 1e-300))
    print("ratios: " + " ".join(f"{q:.2f}" for q in ratios) + f"  median {statistics.median(ratios):.3f}")
    assert statistics.median(ratios) < RATIO_BAR


def _two_part(t):
    """hi + mid of the 3-way split, in float64 (what a 2-part split would feed the products)."""
    hi = t.bfloat16().float()
    mid = (t - hi).bfloat16().float()
    return hi.double() + mid.double()


@pytest.mark.parametrize("shape", ["c40_m72_k7_t203", "c64_m48_k11_t512"])
def test_cancellation_needs_three_parts(shape, device):
    """Negative control: on the cancellation inputs, a 2-part split emulated on the CPU (every product of hi + mid
    operands, summed in float64) misses the bar that the 3-part kernel meets."""
    s, t = SHAPES[shape], _inputs(shape, "cancel")
    ref = _ref(shape, "plain", "cancel")
    two = _conv64(s, _two_part(t["x"]), _two_part(t["w"]))
    err2 = float((two - ref).abs().max() / ref.abs().max())
    r = _run(shape, "plain", "cancel")
    print(f"2-part emulation {err2:.3e}, split kernel {r['err']:.3e}, fp32 kernel {r['err_fp32']:.3e}")
    assert err2 > RTOL, "the case does not separate two parts from three"
    assert r["err"] <= RTOL


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "weight_norm"])
@pytest.mark.parametrize("cin,cout,k", [(24, 136, 3), (33, 24, 5)], ids=["c24_m136_k3", "c33_m24_k5"])
def test_first_part_is_the_bf16_image(cin, cout, k, scaled, device):
    """One layout, one owner: the hi part of the split image, bf16_rne(w * scale), is the bf16 kernel's image byte for
    byte (padded rows at the 128- and the 32-row tile, a partial and a one-channel-tail channel chunk)."""
    g = torch.Generator().manual_seed(cin * 1000 + cout * 10 + k)
    w = torch.randn(cout, cin, k, generator=g).to(device)
    scale = (torch.rand(cout, generator=g) + 0.5).to(device) if scaled else None
    desc = ops.make_conv_desc(1, cin, cout, 64, 64, k, pad_left=(k - 1) // 2)
    image, parts = ops.pack_weight_bf16(desc, w, scale), ops.pack_weight_split(desc, w, scale)
    assert parts.numel() == 3 * image.numel()
    assert torch.equal(parts[:image.numel()], image)
