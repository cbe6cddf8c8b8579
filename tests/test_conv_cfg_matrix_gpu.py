"""GPU: every tile configuration x staging path of the conv forward (``ops.conv1d_forward_cfg``) on shapes whose row
blocks and column tiles are ragged in every tile size, with every fused epilogue term, against a float64 CPU
reference; plus the data gradient of the same shapes on the planner's own configuration.

What the launches of one shape have in common is what the three epilogues of csrc/conv1d.hip (the DMA kernel's
LDS-transposed 16-byte epilogue, the DMA kernel's scalar epilogue, the register-staged kernel's epilogue) and the
split-reduction finish kernel must agree on:

  * values: ``post_act((conv(pre_act(x)) + bias + add1 + add2) * out_mul / out_div)`` within RTOL of float64;
  * stores: the output is a view in the middle of a larger buffer that holds a NaN-payload sentinel; after the launch
    the guard bands on both sides are bit-identical to the sentinel (a ragged tile wrote only its own elements) and
    no element of the output still is the sentinel (every element was written);
  * alignment: an addend or an output that starts 4 bytes off a 16-byte boundary turns the 16-byte epilogue off, and
    the scalar epilogue must then give the SAME BITS (the kernel promises the same arithmetic in the same order);
  * refusals: which (shape, configuration, staging path) triples the library refuses is a literal table.

Chunk-count coverage of the stride-1 shapes (the transposition scratch aliases the dead chunk buffer at an address
that depends on the parity of the chunk count): Cin = 3 / 20 / 32 / 72 give chunk counts 1 / 5 / 8 / 18 at chunk
length 4, 1 / 3 / 4 / 9 at length 8 and 1 / 2 / 2 / 5 at length 16, i.e. a single chunk, an odd count >= 2 and an even
count >= 2 for every chunk length."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from parallelwavegan_amd import _lib, ops
from tests.util import poison_empty, poison_lds

pytestmark = pytest.mark.gpu

# the project's fp32 bound relative to the largest reference magnitude (tests/test_conv_ops_gpu.py); every reduction
# here is at most 504 products long
RTOL = 3e-5
GUARD = 64                     # floats of guard band on each side of an output view (256 B: keeps the view 16-B aligned)
SENTINEL = 0x7FC5A5A5          # a quiet NaN with a payload no kernel produces
NUM_CFGS = 20

# B, Cin, Cout, T_in, T_out, k, stride, dilation, pad_left, groups + form
SHAPES = {
    # rows ragged in every tile (40), Cin no multiple of 4 / 8 / 16, T % 4 == 0 but T % 32 != 0
    "S1": dict(B=2, cin=20, cout=40, t_in=132, t_out=132, k=7, stride=1, dil=3, pad=9, groups=1),
    # a single chunk (the scratch sits behind the buffers), 136 rows; 260: 16-byte epilogue, 259: scalar
    "S2": dict(B=1, cin=3, cout=136, t_in=260, t_out=260, k=3, stride=1, dil=1, pad=1, groups=1),
    "S2b": dict(B=1, cin=3, cout=136, t_in=259, t_out=259, k=3, stride=1, dil=1, pad=1, groups=1),
    # exact tiles everywhere, 1 x 1
    "S3": dict(B=3, cin=32, cout=128, t_in=512, t_out=512, k=1, stride=1, dil=1, pad=0, groups=1),
    # 96 rows; the planner splits the reduction (see test_split_plan_full_epilogue)
    "S4": dict(B=2, cin=72, cout=96, t_in=100, t_out=100, k=5, stride=1, dil=1, pad=2, groups=1),
    # strided and grouped
    "S5": dict(B=2, cin=48, cout=96, t_in=130, t_out=65, k=4, stride=2, dil=1, pad=1, groups=2),
    # transposed: four output phases, out_off != 0, always the scalar epilogue
    "S6": dict(B=2, cin=24, cout=20, t_in=33, t_out=132, k=8, stride=4, dil=1, pad=2, groups=1, transposed=True),
    # the (k, 1) Conv2d form, width 3
    "S7": dict(B=2, cin=24, cout=40, t_in=21, t_out=7, k=5, stride=3, dil=1, pad=2, groups=1, width=3),
    # pad_left = t_in - 1 under reflect / replicate padding: register path only
    "S8r": dict(B=2, cin=20, cout=40, t_in=28, t_out=28, k=3, stride=1, dil=27, pad=27, groups=1, pad_mode="reflect"),
    "S8e": dict(B=2, cin=20, cout=40, t_in=28, t_out=28, k=3, stride=1, dil=27, pad=27, groups=1, pad_mode="replicate"),
}

# bias, add1, add2, out_mul, out_div, post_act, post_slope, pre_act, pre_slope
VARIANTS = {
    "plain": dict(bias=False),
    "res_lrelu": dict(add1=True, post_act="leaky_relu", post_slope=0.2, pre_act="leaky_relu", pre_slope=0.1),
    "mrf": dict(add1=True, add2=True, out_div=3.0, post_act="tanh", pre_act="leaky_relu", pre_slope=0.1),
    "add2_mul": dict(add2=True, out_mul=math.sqrt(0.5), pre_act="relu"),
    "slope0": dict(pre_act="leaky_relu", pre_slope=0.0),   # the generic pre-activation instantiation
    # out_mul under the one post-activation that does not commute with a scale (leaky_relu(s * v) = s * leaky_relu(v))
    "mul_tanh": dict(out_mul=math.sqrt(0.5), post_act="tanh"),
}

# The (shape, tile configuration, use_dma) triples that conv1d_forward_cfg refuses with PWG_ERR_UNSUPPORTED, for the
# only two reasons it may: more than 160 KiB of LDS (S7: the 32 x 512 x 16 tile's double-buffered x window of
# 172 rows x stride 3 x width 3), and the DMA path under a pad mode (all of S8).
REFUSED = {("S7", 8, True)} | {(s, c, True) for s in ("S8r", "S8e") for c in range(20)}
# the configurations on choose_cfg's candidate lists
PLANNER_CFGS = (0, 2, 5, 6, 9, 10, 11, 12, 13, 14, 15, 16, 17)


def _variant(name):
    v = dict(bias=True, add1=False, add2=False, out_mul=1.0, out_div=1.0, post_act=None, post_slope=0.0, pre_act=None,
             pre_slope=0.0)
    v.update(VARIANTS[name])
    return v


def _act(t, act, slope):
    if act == "leaky_relu":
        return F.leaky_relu(t, slope)
    if act == "relu":
        return F.relu(t)
    if act == "tanh":
        return torch.tanh(t)
    return t


def _conv64(s, x, w):
    """The bare convolution of shape ``s`` in float64 (x already pre-activated; autograd-capable)."""
    if s.get("transposed"):
        out_pad = s["t_out"] - ((s["t_in"] - 1) * s["stride"] - 2 * s["pad"] + s["k"])
        return F.conv_transpose1d(x, w, None, stride=s["stride"], padding=s["pad"], output_padding=out_pad,
                                  groups=s["groups"])
    if s.get("width", 1) > 1:
        W = s["width"]
        y = F.conv2d(x.reshape(s["B"], s["cin"], s["t_in"], W), w.unsqueeze(-1), None, stride=(s["stride"], 1),
                     padding=(s["pad"], 0))
        return y.reshape(s["B"], s["cout"], s["t_out"] * W)
    need = (s["t_out"] - 1) * s["stride"] + (s["k"] - 1) * s["dil"] + 1
    right = max(need - s["pad"] - s["t_in"], 0)
    mode = s.get("pad_mode", "zero")
    xp = F.pad(x, (s["pad"], right), mode="constant" if mode == "zero" else mode)
    y = F.conv1d(xp, w, None, stride=s["stride"], dilation=s["dil"], groups=s["groups"])
    return y[..., :s["t_out"]]


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """CPU float32 inputs of a shape, shared (read-only) by every test of that shape."""
    s = SHAPES[shape]
    W = s.get("width", 1)
    g = torch.Generator().manual_seed(sum(map(ord, shape)) * 131 + s["cin"])
    cin_g, cout_g = s["cin"] // s["groups"], s["cout"] // s["groups"]
    x = torch.randn(s["B"], s["cin"], s["t_in"] * W, generator=g)
    wshape = (s["cin"], cout_g, s["k"]) if s.get("transposed") else (s["cout"], cin_g, s["k"])
    taps = s["k"] / s["stride"] if s.get("transposed") else s["k"]
    w = torch.randn(wshape, generator=g) / (cin_g * taps) ** 0.5
    bias = torch.randn(s["cout"], generator=g)
    add1 = torch.randn(s["B"], s["cout"], s["t_out"] * W, generator=g)
    add2 = torch.randn(s["B"], s["cout"], s["t_out"] * W, generator=g)
    # data gradient: dy, an accumulation target, and a forward input that holds exact zeros (mask edge)
    dy = torch.randn(s["B"], s["cout"], s["t_out"] * W, generator=g)
    accum = torch.randn(s["B"], s["cin"], s["t_in"] * W, generator=g)
    xz = torch.randn(s["B"], s["cin"], s["t_in"] * W, generator=g)
    xz[torch.rand(xz.shape, generator=g) < 0.1] = 0.0
    return dict(x=x, w=w, bias=bias, add1=add1, add2=add2, dy=dy, accum=accum, xz=xz)


@functools.lru_cache(maxsize=None)
def _conv_ref(shape, pre_act, pre_slope):
    t = _inputs(shape)
    return _conv64(SHAPES[shape], _act(t["x"].double(), pre_act, pre_slope), t["w"].double())


@functools.lru_cache(maxsize=None)
def _forward_ref(shape, variant):
    """float64 reference of (shape, epilogue variant), computed once."""
    t, v = _inputs(shape), _variant(variant)
    y = _conv_ref(shape, v["pre_act"], v["pre_slope"])
    if v["bias"]:
        y = y + t["bias"].double().view(1, -1, 1)
    if v["add1"]:
        y = y + t["add1"].double()
    if v["add2"]:
        y = y + t["add2"].double()
    y = y * float(torch.tensor(v["out_mul"], dtype=torch.float32)) / v["out_div"]
    return _act(y, v["post_act"], v["post_slope"])


def _desc(shape, v):
    s = SHAPES[shape]
    return ops.make_conv_desc(s["B"], s["cin"], s["cout"], s["t_in"], s["t_out"], s["k"], s["stride"], s["dil"], s["pad"],
                              s["groups"], transposed=s.get("transposed", False), width=s.get("width", 1),
                              pad_mode=s.get("pad_mode", "zero"), pre_act=v["pre_act"], pre_slope=v["pre_slope"],
                              post_act=v["post_act"], post_slope=v["post_slope"], out_mul=v["out_mul"], out_div=v["out_div"])


class Guarded:
    """An output view of ``shape`` in the middle of a sentinel-filled buffer, ``off`` floats past a 16-byte boundary."""

    def __init__(self, shape, device, off=0):
        n = math.prod(shape)
        self.buf = torch.full((GUARD + off + n + GUARD,), SENTINEL, dtype=torch.int32, device=device)
        self.lo, self.hi = GUARD + off, GUARD + off + n
        self.out = self.buf[self.lo:self.hi].view(torch.float32).view(shape)
        assert self.out.data_ptr() % 16 == 4 * off

    def check(self, what):
        assert bool((self.buf[:self.lo] == SENTINEL).all()), f"{what}: store below the output"
        assert bool((self.buf[self.hi:] == SENTINEL).all()), f"{what}: store past the output"
        left = int((self.buf[self.lo:self.hi] == SENTINEL).sum())
        assert left == 0, f"{what}: {left} output elements never written"
        return self.out


def _off4(t):
    """A copy of ``t`` that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _rel_err(y, ref_dev, scale):
    return float((y.double() - ref_dev).abs().max()) / scale


def _refused(e):
    return "status -2" in str(e)


def _dev(shape, device, *names):
    t = _inputs(shape)
    return [t[n].to(device) for n in names]


FORWARD_CASES = [(s, v) for s in SHAPES for v in VARIANTS]


@pytest.mark.parametrize("shape,variant", FORWARD_CASES, ids=[f"{s}-{v}" for s, v in FORWARD_CASES])
def test_every_tile_config(shape, variant, device):
    """All 20 tile configurations x (DMA, register) staging on one (shape, epilogue variant): values against float64,
    guard bands intact, every output element written, and exactly the refusals of the table."""
    s, v = SHAPES[shape], _variant(variant)
    desc = _desc(shape, v)
    x, w, bias, add1, add2 = _dev(shape, device, "x", "w", "bias", "add1", "add2")
    bias, add1, add2 = (bias if v["bias"] else None), (add1 if v["add1"] else None), (add2 if v["add2"] else None)
    ref = _forward_ref(shape, variant).to(device)
    scale = float(ref.abs().max()) + 1e-12
    assert ops.num_tile_configs() == NUM_CFGS
    refused, worst = set(), (0.0, None)
    with poison_lds(), poison_empty():
        wp = ops.pack_weight(desc, w)
        for cfg in range(NUM_CFGS):
            for dma in (True, False):
                what = f"{shape} {variant} cfg {cfg} dma={dma}"
                gd = Guarded(tuple(ref.shape), device)
                try:
                    ops.conv1d_forward_cfg(desc, x, wp, bias, add1, add2, out=gd.out, tile_config=cfg, use_dma=dma)
                except RuntimeError as e:
                    if not _refused(e):
                        raise
                    refused.add((shape, cfg, dma))
                    continue
                y = gd.check(what)
                err = _rel_err(y, ref, scale)
                worst = max(worst, (err, what))
                assert err <= RTOL, f"{what}: rel-to-max error {err:.3e}"
    print(f"worst rel-to-max error {worst[0]:.3e} ({worst[1]})")
    assert refused == {r for r in REFUSED if r[0] == shape}, sorted(refused ^ {r for r in REFUSED if r[0] == shape})
    if shape in ("S1", "S2", "S2b", "S3", "S4"):
        assert not refused, sorted(refused)
    if s.get("pad_mode", "zero") == "zero":
        assert not [r for r in refused if r[2] and r[1] in PLANNER_CFGS], sorted(refused)


ALIGN_CASES = [(s, v) for s in ("S1", "S2", "S3") for v in ("res_lrelu", "mrf")]


@pytest.mark.parametrize("shape,variant", ALIGN_CASES, ids=[f"{s}-{v}" for s, v in ALIGN_CASES])
def test_misaligned_views_give_the_same_bits(shape, variant, device):
    """DMA path, every configuration: ``add1`` as a view 4 bytes off a 16-byte boundary, then the output 4 bytes off,
    both turn the 16-byte epilogue off; the scalar epilogue must reproduce the aligned launch bit for bit."""
    v = _variant(variant)
    desc = _desc(shape, v)
    x, w, bias, add1, add2 = _dev(shape, device, "x", "w", "bias", "add1", "add2")
    add2 = add2 if v["add2"] else None
    add1_off = _off4(add1)
    oshape = tuple(add1.shape)
    with poison_lds(), poison_empty():
        wp = ops.pack_weight(desc, w)
        for cfg in range(NUM_CFGS):
            what = f"{shape} {variant} cfg {cfg}"
            runs = []
            for a1, off in ((add1, 0), (add1_off, 0), (add1, 1)):
                gd = Guarded(oshape, device, off)
                ops.conv1d_forward_cfg(desc, x, wp, bias, a1, add2, out=gd.out, tile_config=cfg, use_dma=True)
                runs.append(gd.check(what))
            assert torch.equal(runs[0], runs[1]), f"{what}: misaligned add1 changes {int((runs[0] != runs[1]).sum())} values"
            assert torch.equal(runs[0], runs[2]), f"{what}: misaligned out changes {int((runs[0] != runs[2]).sum())} values"


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_split_plan_full_epilogue(variant, device):
    """S4 through ``ops.conv1d_forward``: the planner cuts its reduction in two, so the finish kernel applies every
    epilogue term; aligned and misaligned (finish kernel: elementwise, so bit-identical)."""
    v = _variant(variant)
    desc = _desc("S4", v)
    plan = ops.conv1d_plan(desc, has_addends=v["add1"] or v["add2"])
    assert plan["family"] == "mfma" and plan["ksplit"] == 2, plan
    x, w, bias, add1, add2 = _dev("S4", device, "x", "w", "bias", "add1", "add2")
    bias, add1, add2 = (bias if v["bias"] else None), (add1 if v["add1"] else None), (add2 if v["add2"] else None)
    ref = _forward_ref("S4", variant).to(device)
    scale = float(ref.abs().max()) + 1e-12
    with poison_lds(), poison_empty(), ops.profile() as prof:
        wp = ops.pack_weight(desc, w)
        gd = Guarded(tuple(ref.shape), device)
        ops.conv1d_forward(desc, x, wp, bias, add1, add2, out=gd.out)
        y = gd.check("split")
        gd1 = Guarded(tuple(ref.shape), device, 1)
        ops.conv1d_forward(desc, x, wp, bias, add1, _off4(add2) if add2 is not None else None, out=gd1.out)
        y1 = gd1.check("split, misaligned")
    assert "splitk_finish_kernel" in prof.results, sorted(prof.results)
    err = _rel_err(y, ref, scale)
    print(f"rel-to-max error {err:.3e}")
    assert err <= RTOL, f"split {variant}: rel-to-max error {err:.3e}"
    assert torch.equal(y, y1)


# ---- data gradient on the planner's own configuration -----------------------------------------------------------
BWD_SHAPES = ("S1", "S2", "S2b", "S3", "S4", "S5", "S6", "S7")
BWD_MODES = {"lrelu_accum": ("leaky_relu", 0.1, True), "relu_accum": ("relu", 0.0, True), "bare": (None, 0.0, False)}
# the shapes whose data gradient the planner runs as reduction slices + the finish kernel (mask and accum applied there);
# the others apply them in the convolution kernel's own epilogues
BWD_SPLIT = ("S2", "S2b", "S3", "S4", "S5")


@functools.lru_cache(maxsize=None)
def _backward_ref(shape, mode):
    """float64 autograd of conv(pre_act(x)) at the zero-holding x, plus the accumulation target."""
    t = _inputs(shape)
    pre_act, pre_slope, accum = BWD_MODES[mode]
    xz = t["xz"].double().requires_grad_()
    _conv64(SHAPES[shape], _act(xz, pre_act, pre_slope), t["w"].double()).backward(t["dy"].double())
    return xz.grad + t["accum"].double() if accum else xz.grad


BWD_CASES = [(s, m) for s in BWD_SHAPES for m in BWD_MODES]


@pytest.mark.parametrize("shape,mode", BWD_CASES, ids=[f"{s}-{m}" for s, m in BWD_CASES])
def test_data_gradient(shape, mode, device):
    """``ops.conv1d_backward_data`` with the pre-activation mask (x holds exact zeros: the mask is x > 0 ? 1 : slope)
    and ``accum``, and with neither: float64 autograd, guard bands, and misaligned ``accum`` / ``out`` bit-identical
    to the aligned call."""
    pre_act, pre_slope, with_accum = BWD_MODES[mode]
    v = _variant("plain")
    v.update(pre_act=pre_act, pre_slope=pre_slope)
    desc = _desc(shape, v)
    dy, w, xz, accum = _dev(shape, device, "dy", "w", "xz", "accum")
    xm = xz if pre_act is not None else None
    accum = accum if with_accum else None
    ref = _backward_ref(shape, mode).to(device)
    scale = float(ref.abs().max()) + 1e-12
    oshape = tuple(ref.shape)
    split = _lib.lib().pwg_conv1d_backward_data_workspace_floats(ctypes.byref(desc)) > 0
    assert split == (shape in BWD_SPLIT), "the case no longer exercises the epilogue it is here for"
    with poison_lds(), poison_empty():
        wb = ops.pack_weight_bwd(desc, w)
        gd = Guarded(oshape, device)
        ops.conv1d_backward_data(desc, dy, wb, xm, accum, out=gd.out)
        dx = gd.check(f"{shape} {mode}")
        gd_o = Guarded(oshape, device, 1)
        ops.conv1d_backward_data(desc, dy, wb, xm, accum, out=gd_o.out)
        dx_o = gd_o.check(f"{shape} {mode} misaligned out")
        if with_accum:
            gd_a = Guarded(oshape, device)
            ops.conv1d_backward_data(desc, dy, wb, xm, _off4(accum), out=gd_a.out)
            dx_a = gd_a.check(f"{shape} {mode} misaligned accum")
    err = _rel_err(dx, ref, scale)
    print(f"rel-to-max error {err:.3e}")
    assert err <= RTOL, f"{shape} {mode}: rel-to-max error {err:.3e}"
    assert torch.equal(dx, dx_o), f"misaligned out changes {int((dx != dx_o).sum())} values"
    if with_accum:
        assert torch.equal(dx, dx_a), f"misaligned accum changes {int((dx != dx_a).sum())} values"


def test_split_plan_without_enough_workspace(device):
    """S4 through the C entry point itself (``ops.conv1d_forward`` always brings the workspace the query asks for): with
    no workspace, and with one a float short of the query, the dispatcher drops the plan's two reduction slices and
    launches the best unsplit tile instead -- same bound, same guard bands, and the same bits either way."""
    v = _variant("mrf")
    desc = _desc("S4", v)
    lib = _lib.lib()
    need = lib.pwg_conv1d_forward_workspace_floats(ctypes.byref(desc))
    assert ops.conv1d_plan(desc, has_addends=True)["ksplit"] == 2 and need > 1
    x, w, bias, add1, add2 = _dev("S4", device, "x", "w", "bias", "add1", "add2")
    ref = _forward_ref("S4", "mrf").to(device)
    scale = float(ref.abs().max()) + 1e-12
    short = torch.empty(need - 1, device=device, dtype=torch.float32)
    outs = []
    with poison_lds(), poison_empty(), ops.profile() as prof:
        wp = ops.pack_weight(desc, w)
        for what, ws, ws_n in (("NULL workspace", None, need), ("workspace one float short", short, need - 1)):
            gd = Guarded(tuple(ref.shape), device)
            rc = lib.pwg_conv1d_forward(ctypes.byref(desc), ops._ptr(x), ops._ptr(wp), ops._ptr(bias), ops._ptr(add1),
                                        ops._ptr(add2), ops._ptr(gd.out), ops._ptr(ws), ws_n, ops._stream())
            assert rc == 0, f"{what}: status {rc}: {lib.pwg_last_error().decode(errors='replace')}"
            y = gd.check(what)
            err = _rel_err(y, ref, scale)
            print(f"{what}: rel-to-max error {err:.3e}")
            assert err <= RTOL, f"{what}: rel-to-max error {err:.3e}"
            outs.append(y)
    assert "splitk_finish_kernel" not in prof.results, sorted(prof.results)
    assert torch.equal(outs[0], outs[1])
