"""GPU: the batched epilogue and the straight-line staging of the split-operand convolution (csrc/conv1d_split.hip),
at the shapes at which a pipeline over chunks and taps can go wrong as well, with the harness of tests/test_conv_split_gpu.py: a float64 CPU convolution of the same fp32
operands, error relative to the largest reference magnitude, the bar is that file's RTOL = 3e-5, and the output is a
view inside a sentinel-filled buffer.

The shapes (tools/hash_conv_split.py::PIPELINE_SHAPES, which hashes the same cases) are the smallest at which each
piece can go wrong: one / two / three chunks with a channel tail, one tap, a halo on the left only, every row tile with
padded rows, window shifts 0 .. 3, T % 4 != 0 (4-byte staging and the 4-byte epilogue) and T under one tile.  Every
switch of the epilogue and both activations run alone and all together.  Every launch is repeated (same bits), runs at
tile_mode 0 / 1 / 2 (same bits: this also sets interior tiles against edge tiles on the same columns) and once on the
32x32x16 MFMA (within RTOL).  Each of x / add1 / add2 / out passed 4 bytes off a 16-byte boundary must give the bits of
the aligned launch."""
import functools

import pytest
import torch
import torch.nn.functional as F

from parallelwavegan_amd import ops
from tests.test_conv_split_gpu import GUARD, RTOL, SENTINEL, Guarded
from tests.util import poison_empty, poison_lds
from tools.hash_conv_split import (ALIGN_SHAPES, PIPELINE_CASES, PIPELINE_SHAPES, off_by_4_bytes, pipeline_desc,
                                   pipeline_inputs, pipeline_variant)

pytestmark = pytest.mark.gpu

IDS = [f"{s}-{v}-{kind}" for s, v, kind in PIPELINE_CASES]
_inputs = functools.lru_cache(maxsize=None)(pipeline_inputs)


def _act(t, act, slope=0.0):
    if act == "leaky_relu":
        return F.leaky_relu(t, slope)
    if act == "relu":
        return F.relu(t)
    if act == "tanh":
        return torch.tanh(t)
    return t


@functools.lru_cache(maxsize=None)
def _conv_ref(shape, kind, pre_act, pre_slope):
    """The bare convolution in float64 (the pre-activation is applied in fp32, as the kernel defines it)."""
    s, t = PIPELINE_SHAPES[shape], _inputs(shape, kind)
    halo = (s["k"] - 1) * s["dil"]
    xp = F.pad(_act(t["x"], pre_act, pre_slope).double(), (s["pad_left"], halo - s["pad_left"]))
    w = t["w"].double()
    y = torch.zeros(s["B"], s["cout"], s["T"], dtype=torch.float64)
    for tap in range(s["k"]):
        y += torch.matmul(w[:, :, tap], xp[:, :, tap * s["dil"]:tap * s["dil"] + s["T"]])
    return y


@functools.lru_cache(maxsize=None)
def _ref(shape, variant, kind):
    t, v = _inputs(shape, kind), pipeline_variant(variant)
    y = _conv_ref(shape, kind, v["pre_act"], v["pre_slope"])
    if v["bias"]:
        y = y + t["bias"].double().view(1, -1, 1)
    if v["add1"]:
        y = y + t["add1"].double()
    if v["add2"]:
        y = y + t["add2"].double()
    return _act(y * v["out_mul"] / v["out_div"], v["post_act"], v["post_slope"])


@functools.lru_cache(maxsize=None)
def _run(shape, variant, kind):
    device = torch.device("cuda:0")
    v, t = pipeline_variant(variant), _inputs(shape, kind)
    desc = pipeline_desc(shape, variant)
    assert ops.conv1d_split_supported(desc)
    x, w = t["x"].to(device), t["w"].to(device)
    bias, add1, add2 = (t[n].to(device) if v[n] else None for n in ("bias", "add1", "add2"))
    ref = _ref(shape, variant, kind).to(device)
    scale = float(ref.abs().max()) + 1e-300
    what = f"{shape} {variant} {kind}"

    def err(y):
        return float((y.double() - ref).abs().max()) / scale

    def split(**cfg):
        gd = Guarded(tuple(ref.shape), device)
        ops.conv1d_forward_split(desc, x, ws, bias, add1, add2, out=gd.out, **cfg)
        return gd.check(f"{what} {cfg}")

    with poison_lds(), poison_empty():
        ws = ops.pack_weight_split(desc, w)
        y, again = split(), split()
        full, half = split(tile_mode=1), split(tile_mode=2)
        y32 = split(mfma_shape=32)
    return dict(err=err(y), err32=err(y32), repeat=torch.equal(y, again),
                tiles=torch.equal(y, full) and torch.equal(y, half))


@pytest.mark.parametrize("shape,variant,kind", PIPELINE_CASES, ids=IDS)
def test_split_pipeline(shape, variant, kind, device):
    r = _run(shape, variant, kind)
    print(f"rel-to-max error: 16x16x32 {r['err']:.3e}  32x32x16 {r['err32']:.3e}")
    assert r["err"] <= RTOL, f"rel-to-max error {r['err']:.3e}"
    assert r["err32"] <= RTOL, f"32x32x16: rel-to-max error {r['err32']:.3e}"
    assert r["repeat"], "two launches on the same inputs differ"
    assert r["tiles"], "tile_mode 0 / 1 / 2 differ"


@pytest.mark.parametrize("which", ["x", "add1", "add2", "out"])
@pytest.mark.parametrize("shape", ALIGN_SHAPES)
def test_operand_off_16_byte_boundary(shape, which, device):
    """One operand 4 bytes off a 16-byte boundary (x: 4-byte staging; add1 / add2 / out: the epilogue's 4-byte path)
    gives the bits of the aligned launch, within its guard bands."""
    t = _inputs(shape, "randn")
    desc = pipeline_desc(shape, "all")
    arg = {n: t[n].to(device) for n in ("x", "bias", "add1", "add2")}
    oshape = tuple(t["add1"].shape)
    with poison_lds(), poison_empty():
        ws = ops.pack_weight_split(desc, t["w"].to(device))
        aligned = Guarded(oshape, device)
        assert all(p.data_ptr() % 16 == 0 for p in (arg["x"], arg["add1"], arg["add2"], aligned.out))
        ops.conv1d_forward_split(desc, arg["x"], ws, arg["bias"], arg["add1"], arg["add2"], out=aligned.out)
        want = aligned.check(f"{shape} aligned")
        if which == "out":  # the output starts one float into a sentinel-filled span
            n = want.numel()
            buf = torch.full((GUARD + 1 + n + GUARD,), SENTINEL, dtype=torch.int32, device=device)
            out = buf[GUARD + 1:GUARD + 1 + n].view(torch.float32).view(oshape)
            assert out.data_ptr() % 16 == 4
            ops.conv1d_forward_split(desc, arg["x"], ws, arg["bias"], arg["add1"], arg["add2"], out=out)
            assert bool((buf[:GUARD + 1] == SENTINEL).all()), "store below the shifted output"
            assert bool((buf[GUARD + 1 + n:] == SENTINEL).all()), "store past the shifted output"
            assert int((buf[GUARD + 1:GUARD + 1 + n] == SENTINEL).sum()) == 0, "output elements never written"
        else:
            arg[which] = off_by_4_bytes(arg[which])
            assert arg[which].data_ptr() % 16 == 4
            gd = Guarded(oshape, device)
            ops.conv1d_forward_split(desc, arg["x"], ws, arg["bias"], arg["add1"], arg["add2"], out=gd.out)
            out = gd.check(f"{shape} {which} off by 4 bytes")
    assert torch.equal(out, want), f"{which} 4 bytes off a 16-byte boundary changes the result"
