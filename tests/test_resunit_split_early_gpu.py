"""GPU: the EARLY epilogue operands of the split-operand residual unit (csrc/resunit_split.hip).  The kernel requests the
raw-x residual of a lane's own output values behind the window's staging loads, and add2 ahead of its last contraction,
and holds both in registers until the epilogue.  What can go wrong is an address: the row base of the batch entry, the
clamp of a value that is not stored to the tile's first samples, the tile's first output sample.  Lengths that put those
loads on every edge they have (batch 2, so that the row base counts):

  T = 64            one tile, most value groups not stored: their loads read the clamped address
  T = bn_out + 4    a second tile with a single stored value group
  T = 2 * bn_out    no ragged tile

with bn_out = (H - (k - 1)) & ~3, H = 256 at C = 32 and 128 at C = 64, the outputs per tile of the pair form; the single
form (bn_out = H) also runs T = H + 4 and 2 * H, its own tile edges.  C = 32 / 64, (k, d) = (3, 1) / (11, 5), pair and
single form, both MFMA shapes; add2 absent, add2 present with out_div = 3, and add2 aliasing the output (a lane reads only
the elements it later writes).  The oracle is the chain of two ``ops.conv1d_forward_split`` launches (one for the single
form) with ``torch.equal``; every launch runs under poisoned LDS into a poisoned, guarded output and is repeated."""
import functools
import itertools

import pytest
import torch

from parallelwavegan_amd import ops
from tests.test_conv_split_gpu import SENTINEL, Guarded
from tests.util import poison_empty, poison_lds

pytestmark = pytest.mark.gpu

B = 2
SLOPE = 0.1
H = {32: 256, 64: 128}


def _lengths(c, k, pair):
    bn_pair = (H[c] - (k - 1)) & ~3
    ts = [64, bn_pair + 4, 2 * bn_pair]
    if not pair:
        ts += [H[c] + 4, 2 * H[c]]
    return ts


# (C, k, d, pair, T, variant)
CASES = [(c, k, d, pair, t, v)
         for c, (k, d), pair in itertools.product((32, 64), ((3, 1), (11, 5)), (True, False))
         for t in _lengths(c, k, pair) for v in ("plain", "add2_div3", "add2_is_y")]
IDS = ["c%d_k%d_d%d_%s_t%d-%s" % (c, k, d, "pair" if p else "single", t, v) for c, k, d, p, t, v in CASES]


@functools.lru_cache(maxsize=None)
def _inputs(c, k, t):
    g = torch.Generator().manual_seed(c * 7919 + k * 131 + t)
    return dict(x=torch.randn(B, c, t, generator=g), w1=torch.randn(c, c, k, generator=g) / (c * k) ** 0.5,
                w2=torch.randn(c, c, k, generator=g) / (c * k) ** 0.5, b1=torch.randn(c, generator=g),
                b2=torch.randn(c, generator=g), add2=torch.randn(B, c, t, generator=g))


@pytest.mark.parametrize("mfma_shape", [16, 32])
@pytest.mark.parametrize("c,k,d,pair,t,variant", CASES, ids=IDS)
def test_early_operands(c, k, d, pair, t, variant, mfma_shape, device):
    i = {n: v.to(device) for n, v in _inputs(c, k, t).items()}
    x, b1, b2 = i["x"], i["b1"], i["b2"]
    add2 = None if variant == "plain" else i["add2"]
    out_div = 1.0 if variant == "plain" else 3.0
    pad = (k - 1) // 2
    unit = ops.make_resunit_desc(B, c, t, k, d, pair, SLOPE, SLOPE, out_div)
    assert ops.resunit_split_supported(unit)
    wdesc = ops.make_conv_desc(B, c, c, t, t, k, 1, 1, pad)
    what = f"unit C{c} k{k} d{d} pair{pair} T{t} {variant} {mfma_shape}"

    def launch():
        gd = Guarded((B, c, t), device)
        a2 = add2
        if variant == "add2_is_y":  # the running sum is updated in place
            gd.out.copy_(add2)
            a2 = gd.out
        ops.resunit_forward_split(unit, x, i1, b1, i2 if pair else None, b2 if pair else None, a2, out=gd.out,
                                  mfma_shape=mfma_shape)
        if variant == "add2_is_y":  # (the copy has overwritten every sentinel: only the guards are checked)
            assert bool((gd.buf[:gd.lo] == SENTINEL).all()) and bool((gd.buf[gd.hi:] == SENTINEL).all()), what
            return gd.out
        return gd.check(what)

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
    assert torch.isfinite(chain).all()
    assert torch.equal(y, chain), "the unit differs from the chain of split convolutions"
    assert torch.equal(y, again), "two launches on the same inputs differ"
