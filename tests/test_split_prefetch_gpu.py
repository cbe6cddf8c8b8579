"""GPU: the step SEQUENCE of the split-operand contraction (csrc/mfma_conv.h).  ``resunit_split_kernel`` runs the
streamed form of the reduction step (``split_step_streamed``: the weight fragments are requested a row tile ahead of their
MFMAs, across tap, k-step and chunk boundaries, and ``split_step_successor`` names the step that follows);
``conv1d_split_mfma_kernel`` runs the resident form around the same ``split_product``.  The numerical bars and the chain
identity are held by the existing suites; this file covers what the sequence of steps and row tiles can get wrong in
either form, at the smallest shapes that reach each edge:

  one step in total          c_in = 32 and 24 (a partial chunk), k = 1: the first request ahead is already the clamped one
  a chunk crossing per step  c_in = 72 (3 chunks, the last partial), k = 1
  taps and chunks, dilated   c_in = 40, c_out = 72, k = 3, dilation 5, T = 132
  row tiles                  c_out = 24 (32-row tile, one row tile per wave: the ring wraps every step), 136 (two row
                             blocks of 128, padded rows), 128 (four row tiles per wave); k = 3, c_in = 64, T = 260: two
                             column tiles, the last one ragged, T % 4 == 0

Every convolution case goes through ``pwg_conv1d_split_forward_cfg`` at both MFMA shapes and both tile modes with batch
2: the two tile modes must give the same bits, a repeated launch must give the same bits, and the error against a
float64 convolution of the same fp32 operands stays within 3e-5 of the largest output (RTOL of
tests/test_conv_split_gpu.py).  The units (``ops.resunit_forward_split``; C = 32 / 64, (k, d) = (3, 1) / (11, 5), pair and
single form, T = 64 plain and T = 516 with add2 and out_div = 3) must equal the chain of two
``ops.conv1d_forward_split`` launches bit for bit, and repeat.  Inputs are ``torch.randn`` with fixed seeds."""
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

from parallelwavegan_amd import ops
from tests.test_conv_split_gpu import RTOL, Guarded
from tests.util import poison_empty, poison_lds

pytestmark = pytest.mark.gpu

B = 2
SLOPE = 0.1
# name -> c_in, c_out, T, k, dilation
CONV_CASES = {
    "one_step": (32, 32, 64, 1, 1),
    "one_step_partial_chunk": (24, 32, 64, 1, 1),
    "chunk_crossing_every_step": (72, 64, 64, 1, 1),
    "taps_chunks_dilated": (40, 72, 132, 3, 5),
    "row_tile_32": (64, 24, 260, 3, 1),
    "row_blocks_padded": (64, 136, 260, 3, 1),
    "row_tiles_4": (64, 128, 260, 3, 1),
}
# (C, k, d, pair, T, add2, out_div)
UNIT_CASES = [(c, k, d, pair, t, extra, 3.0 if extra else 1.0)
              for c, (k, d), pair, (t, extra) in itertools.product((32, 64), ((3, 1), (11, 5)), (True, False),
                                                                   ((64, False), (516, True)))]
UNIT_IDS = ["c%d_k%d_d%d_%s_t%d" % (c, k, d, "pair" if p else "single", t) for c, k, d, p, t, _, _ in UNIT_CASES]


@functools.lru_cache(maxsize=None)
def _conv_inputs(name):
    cin, cout, t, k, _ = CONV_CASES[name]
    g = torch.Generator().manual_seed(20240 + sorted(CONV_CASES).index(name))
    return torch.randn(B, cin, t, generator=g), torch.randn(cout, cin, k, generator=g) / (cin * k) ** 0.5


@functools.lru_cache(maxsize=None)
def _conv_ref(name):
    """The 'same' convolution in float64 from the fp32 operands, as k matrix products over shifted views."""
    _, cout, t, k, dil = CONV_CASES[name]
    x, w = _conv_inputs(name)
    pad = (k - 1) // 2 * dil
    xp = F.pad(x.double(), (pad, pad))
    y = torch.zeros(B, cout, t, dtype=torch.float64)
    for tap in range(k):
        y += torch.matmul(w[:, :, tap].double(), xp[:, :, tap * dil:tap * dil + t])
    return y


@pytest.mark.parametrize("mfma_shape", [16, 32])
@pytest.mark.parametrize("name", list(CONV_CASES))
def test_step_sequence_conv(name, mfma_shape, device):
    cin, cout, t, k, dil = CONV_CASES[name]
    x, w = (v.to(device) for v in _conv_inputs(name))
    ref = _conv_ref(name).to(device)
    scale = float(ref.abs().max())
    desc = ops.make_conv_desc(B, cin, cout, t, t, k, 1, dil, (k - 1) // 2 * dil)
    assert ops.conv1d_split_supported(desc)

    def launch(tile_mode):
        gd = Guarded((B, cout, t), device)
        ops.conv1d_forward_split(desc, x, ws, out=gd.out, mfma_shape=mfma_shape, tile_mode=tile_mode)
        return gd.check(f"{name} {mfma_shape} tile_mode {tile_mode}")

    with poison_lds(), poison_empty():
        ws = ops.pack_weight_split(desc, w)
        full, half, again = launch(1), launch(2), launch(1)
    for what, y in (("full-size tiles", full), ("half-size tiles", half)):
        err = float((y.double() - ref).abs().max()) / scale
        print(f"{name} {mfma_shape} {what}: rel-to-max error {err:.3e}")
        assert err <= RTOL, f"{what}: rel-to-max error {err:.3e}"
    assert torch.equal(full, half), "the two tile modes differ"
    assert torch.equal(full, again), "two launches on the same inputs differ"


@functools.lru_cache(maxsize=None)
def _unit_inputs(c, k, t):
    g = torch.Generator().manual_seed(c * 1009 + k * 101 + t)
    return dict(x=torch.randn(B, c, t, generator=g), w1=torch.randn(c, c, k, generator=g) / (c * k) ** 0.5,
                w2=torch.randn(c, c, k, generator=g) / (c * k) ** 0.5, b1=torch.randn(c, generator=g),
                b2=torch.randn(c, generator=g), add2=torch.randn(B, c, t, generator=g))


@pytest.mark.parametrize("mfma_shape", [16, 32])
@pytest.mark.parametrize("c,k,d,pair,t,extra,out_div", UNIT_CASES, ids=UNIT_IDS)
def test_step_sequence_unit(c, k, d, pair, t, extra, out_div, mfma_shape, device):
    i = {n: v.to(device) for n, v in _unit_inputs(c, k, t).items()}
    x, b1, b2 = i["x"], i["b1"], i["b2"]
    add2 = i["add2"] if extra else None
    pad = (k - 1) // 2
    unit = ops.make_resunit_desc(B, c, t, k, d, pair, SLOPE, SLOPE, out_div)
    assert ops.resunit_split_supported(unit)
    wdesc = ops.make_conv_desc(B, c, c, t, t, k, 1, 1, pad)

    def launch():
        gd = Guarded((B, c, t), device)
        ops.resunit_forward_split(unit, x, i1, b1, i2 if pair else None, b2 if pair else None, add2, out=gd.out,
                                  mfma_shape=mfma_shape)
        return gd.check(f"unit C{c} k{k} d{d} pair{pair} T{t} {mfma_shape}")

    with poison_lds(), poison_empty():
        i1, i2 = ops.pack_weight_split(wdesc, i["w1"]), ops.pack_weight_split(wdesc, i["w2"])
        if pair:
            d1 = ops.make_conv_desc(B, c, c, t, t, k, 1, d, pad * d, pre_act="leaky_relu", pre_slope=SLOPE,
                                    post_act="leaky_relu", post_slope=SLOPE)
            d2 = ops.make_conv_desc(B, c, c, t, t, k, 1, 1, pad, out_div=out_div)
            h = ops.conv1d_forward_split(d1, x, i1, b1, mfma_shape=mfma_shape)
            chain = ops.conv1d_forward_split(d2, h, i2, b2, x, add2, mfma_shape=mfma_shape)
        else:
            d1 = ops.make_conv_desc(B, c, c, t, t, k, 1, d, pad * d, pre_act="leaky_relu", pre_slope=SLOPE,
                                    out_div=out_div)
            chain = ops.conv1d_forward_split(d1, x, i1, b1, x, add2, mfma_shape=mfma_shape)
        y, again = launch(), launch()
    assert torch.equal(y, chain), "the unit differs from the chain of two split convolutions"
    assert torch.equal(y, again), "two launches on the same inputs differ"
