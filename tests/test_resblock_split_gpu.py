"""GPU: the chained block of split-operand residual units (``resblock_split_kernel`` of csrc/resunit_split.hip,
``ops.resblock_forward_split``).

The oracle is the chain the kernel is defined by ("The chained block"): N ``ops.resunit_forward_split``
launches at the same MFMA shape, units 0 .. N - 2 without add2 and out_div, the last with the block's, and the comparison
is ``torch.equal``.  Every case also runs against a float64 block of the same fp32 operands (the activation of the
block's input applied in fp32, as tests/test_resunit_split_gpu.py does), error relative to the largest output, gate 3e-5
(the project's fp32 bar).

Shapes: (C, k) = (32, 3), (64, 3), (32, 7); N = 2 and 3 with dilations (1, 3, 5)[:N]; batch 2 - 3; T = 100 (shorter than
one frame's stored columns: both ends of the row inside one frame), bn_out (exactly one frame: 232 / 104 at k = 3,
N = 3), bn_out + 4 (a second frame of 4 columns) and 1000 (a few frames, the last one short).  With the biases on, a
y_u that is not zeroed outside [0, T) changes the columns next to the row's ends: the "all" cases at every T guard the
zero padding between units.  Each launch runs under poisoned LDS and a poisoned output, into a guarded view, twice."""
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

from parallelwavegan_amd import _lib, ops
from tests.test_conv_split_gpu import Guarded
from tests.test_resunit_split_gpu import _conv64
from tests.util import poison_empty, poison_lds

pytestmark = pytest.mark.gpu

RTOL = 3e-5
SLOPES1 = (0.1, 0.2, 0.05)  # per unit: the slope between two units is the NEXT unit's
SLOPES2 = (0.1, 0.15, 0.3)
DILATIONS = (1, 3, 5)
VARIANTS = {
    "plain": dict(bias=False, add2=False, out_div=1.0),
    "all": dict(bias=True, add2=True, out_div=3.0),
    "bias": dict(bias=True, add2=False, out_div=1.0),
    "add2": dict(bias=False, add2=True, out_div=1.0),
    "div3": dict(bias=False, add2=False, out_div=3.0),
}
CK = [(32, 3), (64, 3), (32, 7)]


def _bn_out(c, k, n):
    """Stored columns per frame, by the definition (the host test pins the library's answer to it)."""
    edge = sum((k - 1) // 2 * (d + 1) for d in DILATIONS[:n])
    return (256 if c == 32 else 128) - 2 * ((edge + 3) // 4 * 4)


# (C, k, N, batch, T, variant, kind)
CASES = []
for (c, k), n, v in itertools.product(CK, (2, 3), ("plain", "all")):
    one = _bn_out(c, k, n)
    CASES += [(c, k, n, b, t, v, "randn") for b, t in ((2, 100), (3, one), (2, one + 4), (3, 1000))]
# each epilogue term alone, at a few frames with a short last one
CASES += [(32, 3, 3, 3, 1000, v, "randn") for v in ("bias", "add2", "div3")]
# the input kinds of tests/test_conv_split_gpu.py
CASES += [(64, 3, 3, 3, 1000, "all", "wide"), (32, 7, 2, 3, 1000, "plain", "wide"),
          (32, 3, 3, 3, 1000, "all", "cancel"), (64, 3, 2, 3, 1000, "plain", "cancel")]
IDS = ["c%d_k%d_n%d_b%d_t%d-%s-%s" % case for case in CASES]


@functools.lru_cache(maxsize=None)
def _inputs(c, k, b, t, kind):
    """CPU float32 inputs, shared (read-only) by every case of this size: three units' weights and biases."""
    g = torch.Generator().manual_seed(c * 100003 + k * 1009 + b * 101 + t + len(kind))
    x = torch.randn(b, c, t, generator=g)
    w1 = [torch.randn(c, c, k, generator=g) / (c * k) ** 0.5 for _ in range(3)]
    w2 = [torch.randn(c, c, k, generator=g) / (c * k) ** 0.5 for _ in range(3)]
    if kind == "wide":  # channel magnitudes 2^-20 .. 2^20
        e = torch.linspace(-20, 20, c)[torch.randperm(c, generator=g)]
        x = x * torch.exp2(e.round()).view(1, -1, 1)
    if kind == "cancel":  # w and -w on paired channels of near-equal inputs
        u = torch.rand(b, c // 2, t, generator=g) * 2 - 1
        x[:, 1::2] = x[:, 0::2] * (1 + u / 16)
        w1[0][:, 1::2] = -w1[0][:, 0::2]
    return dict(x=x, w1=w1, w2=w2, b1=[torch.randn(c, generator=g) for _ in range(3)],
                b2=[torch.randn(c, generator=g) for _ in range(3)], add2=torch.randn(b, c, t, generator=g))


@functools.lru_cache(maxsize=None)
def _ref(c, k, n, b, t, variant, kind):
    """The block in float64 from the fp32 operands; lrelu of the block's input is formed in fp32."""
    i, v = _inputs(c, k, b, t, kind), VARIANTS[variant]
    x = i["x"].double()
    for u in range(n):
        a = F.leaky_relu(i["x"], SLOPES1[0]).double() if u == 0 else F.leaky_relu(x, SLOPES1[u])
        h = _conv64(a, i["w1"][u].double(), DILATIONS[u])
        if v["bias"]:
            h = h + i["b1"][u].double().view(1, -1, 1)
        h = _conv64(F.leaky_relu(h, SLOPES2[u]), i["w2"][u].double(), 1)
        if v["bias"]:
            h = h + i["b2"][u].double().view(1, -1, 1)
        x = h + x
    if v["add2"]:
        x = x + i["add2"].double()
    return x / v["out_div"]


@functools.lru_cache(maxsize=None)
def _run(c, k, n, b, t, variant, kind):
    device = torch.device("cuda:0")
    i, v = _inputs(c, k, b, t, kind), VARIANTS[variant]
    x = i["x"].to(device)
    b1 = [i["b1"][u].to(device) if v["bias"] else None for u in range(n)]
    b2 = [i["b2"][u].to(device) if v["bias"] else None for u in range(n)]
    add2 = i["add2"].to(device) if v["add2"] else None
    ref = _ref(c, k, n, b, t, variant, kind).to(device)
    scale = float(ref.abs().max()) + 1e-300
    dil, s1, s2 = DILATIONS[:n], SLOPES1[:n], SLOPES2[:n]
    desc = ops.make_resunit_desc(b, c, t, k, 1, True, s1[0], s2[0], v["out_div"])
    assert ops.resblock_split_supported(desc, dil), _lib.lib().pwg_last_error().decode()
    what = f"C{c} k{k} N{n} B{b} T{t} {variant} {kind}"

    def err(y):
        return float((y.double() - ref).abs().max()) / scale

    def block(shape):
        gd = Guarded(tuple(x.shape), device)
        ops.resblock_forward_split(desc, x, dil, s1, s2, i1, b1, i2, b2, add2, out=gd.out, mfma_shape=shape)
        return gd.check(f"{what} mfma {shape}")

    def chain(shape):
        y = x
        for u in range(n):
            last = u == n - 1
            du = ops.make_resunit_desc(b, c, t, k, dil[u], True, s1[u], s2[u], v["out_div"] if last else 1.0)
            y = ops.resunit_forward_split(du, y, i1[u], b1[u], i2[u], b2[u], add2 if last else None, mfma_shape=shape)
        return y

    wdesc = ops.make_conv_desc(1, c, c, 64, 64, k, pad_left=(k - 1) // 2)
    with poison_lds(), poison_empty():
        i1 = [ops.pack_weight_split(wdesc, i["w1"][u].to(device)) for u in range(n)]
        i2 = [ops.pack_weight_split(wdesc, i["w2"][u].to(device)) for u in range(n)]
        y16, again, y32 = block(16), block(16), block(32)
        default = ops.resblock_forward_split(desc, x, dil, s1, s2, i1, b1, i2, b2, add2)
        c16, c32 = chain(16), chain(32)
    return dict(err=err(y16), err32=err(y32), repeat=torch.equal(y16, again), default=torch.equal(default, y16),
                chain16=torch.equal(y16, c16), chain32=torch.equal(y32, c32),
                diff16=float((y16 - c16).abs().max()), diff32=float((y32 - c32).abs().max()))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_block(case, device):
    r = _run(*case)
    print(f"rel-to-max error: block {r['err']:.3e} (32x32x16: {r['err32']:.3e})  "
          f"|block - chain| {r['diff16']:.3e} / {r['diff32']:.3e}")
    assert r["chain16"], f"16x16x32: differs from the chained unit launches by {r['diff16']:.3e}"
    assert r["chain32"], f"32x32x16: differs from the chained unit launches by {r['diff32']:.3e}"
    assert r["repeat"], "two launches on the same inputs differ"
    assert r["default"], "the default launch is not the 16x16x32 one"
    assert r["err"] <= RTOL, f"rel-to-max error {r['err']:.3e}"
    assert r["err32"] <= RTOL, f"32x32x16: rel-to-max error {r['err32']:.3e}"


def test_profiler_names_the_block(device):
    c, k, t, n = 32, 3, 464, 3
    x = torch.randn(2, c, t, device=device)
    wdesc = ops.make_conv_desc(1, c, c, 64, 64, k, pad_left=1)
    img = [ops.pack_weight_split(wdesc, torch.randn(c, c, k, device=device) / 10) for _ in range(n)]
    desc = ops.make_resunit_desc(2, c, t, k, 1, True)
    with ops.profile() as prof:
        ops.resblock_forward_split(desc, x, DILATIONS, (0.1,) * n, (0.1,) * n, img, [None] * n, img, [None] * n)
    assert [name for name in prof.results if "resblock_split_kernel" in name]
    assert not any("resunit_split_kernel" in name for name in prof.results)


def test_refused_blocks_launch_nothing(device):
    """Every refusal is a host decision with a message: the output keeps its sentinel."""
    c, k, t, n = 32, 3, 64, 3
    x = torch.randn(1, c, t, device=device)
    wdesc = ops.make_conv_desc(1, c, c, 64, 64, k, pad_left=1)
    img = [ops.pack_weight_split(wdesc, torch.randn(c, c, k, device=device))] * n
    ok = ops.make_resunit_desc(1, c, t, k, 1, True)

    def refused(desc, out, match, dil=DILATIONS, **kw):
        before = out.clone()
        m = len(dil)
        with ops.profile() as prof:
            with pytest.raises(RuntimeError, match=match):
                ops.resblock_forward_split(desc, x, dil, (0.1,) * m, (0.1,) * m, img[:m], [None] * m, img[:m],
                                           [None] * m, out=out, **kw)
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), before.view(torch.int32))
        assert not any("resblock_split_kernel" in name for name in prof.results)

    out = torch.full_like(x, float("nan"))
    refused(ok, x, "alias")
    refused(ops.make_resunit_desc(1, c, t, k, 1, False), out, "single-convolution")
    refused(ok, out, "outputs per frame", dil=(9, 27, 27))
    refused(ok, out, "mfma_shape", mfma_shape=8)
    buf = torch.full((c * t + 4,), float("nan"), device=device)
    refused(ok, buf[1:1 + c * t].view(1, c, t), "aligned")
