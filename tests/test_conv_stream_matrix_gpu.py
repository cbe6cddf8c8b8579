"""GPU: the fp32 conv stream kernel (csrc/conv1d_stream.hip) one chunk per launch against the float64 references of
tests/stream_refs.py, each launch on inputs of its OWN (a random ``hist_in``, not the previous launch's output), over a
covering table of the kernel's edges: staged blocks of 64 input channels (one, a ragged second, three, eight), tap
batches of four (1 .. 11 taps; with 9 and 11 a block has three batches and the weight buffer's parity alternates from
block to block), histories from 0 to the cap of 144 columns with chunks shorter and longer than them, the three column
tiles at exact / minus 1 / plus 1 and a ragged last tile, row counts below, at and above the image's 128-row stretch,
the transposed form's row blocks inside and across phases, every epilogue term alone and all together, and the three
start-of-stream paddings.

What every launch has in common:

  * ``y`` within RTOL of float64, relative to the largest reference magnitude;
  * ``hist_out`` (and every delay-line output) equal to the reference bit for bit: it is a copy;
  * every output is a view in the middle of a sentinel-filled buffer (``Guarded``): bands intact, every element written;
  * state the launch must not read is NaN-filled: every state input of a fresh slotted item, x and the addends of a
    paused one (the plain and delayed forms start a stream from a NULL ``hist_in``: there is no buffer to fill);
  * the LDS is NaN-poisoned before every launch;
  * one case per form is launched twice: bit-identical.

The tile a case claims is asserted through ``ops.conv1d_stream_plan`` (here and, without a GPU, in
tests/test_stream_refs_host.py, which also measures the float32 room under RTOL and the sensitivity of every case)."""
import collections
import functools
import math

import pytest
import torch

from parallelwavegan_amd import ops
from tests import stream_refs as R
from tests.test_wavenet_matrix_gpu import Guarded, _place
from tests.util import poison_lds

pytestmark = pytest.mark.gpu

# The project's fp32 bar (RTOL of tests/test_conv_ops_gpu.py), relative to the largest reference magnitude; the longest
# reduction here is 512 x 11 products.  The float32 CPU evaluation of the same formulas on the same data is within
# 1.1e-6 of float64 on every row below (worst 3.7 % of the bar, at tr-16-8-24 n = 9;
# tests/test_stream_refs_host.py::test_room_under_the_bar), so the data leave the bar about 27x of room.
# Measured on an MI355X, worst per form: plain 1.14e-6 (the same row), 32 x 64 tile 1.9e-7, delayed 2.8e-7, slotted
# 1.5e-7, mirrored 7.1e-7.
RTOL = 3e-5
PRE_SLOPE, POST_SLOPE = 0.1, 0.2

# entry point of csrc/conv1d_stream.hip -> the test that drives it directly (checked by tests/test_stream_refs_host.py)
COVERED = {
    "pwg_conv1d_stream_supported": "test_plain_chunk",
    "pwg_conv1d_stream_hist_floats": "test_plain_chunk",
    "pwg_conv1d_stream_plan": "test_plain_chunk",
    "pwg_conv1d_stream_forward": "test_plain_chunk",
    "pwg_conv1d_stream_delayed_supported": "test_delayed_form",
    "pwg_conv1d_stream_delayed_forward": "test_delayed_form",
    "pwg_conv1d_stream_slots_forward": "test_slotted_form",
    "pwg_conv1d_stream_mirrored_supported": "test_mirrored_form",
    "pwg_conv1d_stream_mirrored_forward": "test_mirrored_form",
}

Case = collections.namedtuple("Case", "id cin cout k d ns tiles B s pad start pre bias add1 add2 mul div post")


def C(id, cin, cout, k, d, ns, tiles, B=1, s=0, pad="zero", start=False, pre=None, bias=False, add1=False, add2=False,
      mul=1.0, div=1.0, post=None):
    """A row: a layer (``s``: the stride of a transposed one, k = 2 s), chunk lengths ``ns`` with the column tile each
    claims, batch, start-of-stream padding (``start``: hist_in is NULL), pre-activation and epilogue terms."""
    assert len(ns) == len(tiles) and (not s or (k == 2 * s and d == 1))
    return Case(id, cin, cout, k, d, ns, tiles, B, s, pad, start, pre, bias, add1, add2, mul, div, post)


ALL = dict(bias=True, add1=True, add2=True, mul=math.sqrt(0.5), div=3.0)
CASES = [
    # ---- stride 1
    # c_in 1: one real channel in a 16-channel image, waves 1 - 3 contract nothing; c_out 1; k = 1: H = 0, no history
    # buffers, W = 16 / 32 / 64 divides 256 so the staging loop never carries
    C("cin1-k1", 1, 1, 1, 1, (1, 16, 17, 33), (16, 16, 32, 64), B=2),
    # H = 1; three 16-channel groups exactly (wave 3 idle); bias alone
    C("cin48-k2", 48, 24, 2, 1, (1, 15, 17), (16, 16, 32), B=3, bias=True),
    # one full staged block; the three column tiles exactly; add1 alone
    C("cin64-k3", 64, 40, 3, 1, (16, 32, 64), (16, 32, 64), B=2, add1=True),
    # cin_pad 80: the second block holds one group, half of it padding; exactly four taps (one batch); m = m_pad = 128;
    # tiles minus 1 / plus 1; add2 alone
    C("cin72-k4", 72, 128, 4, 2, (15, 33, 65), (16, 64, 64), add2=True),
    # three blocks, c_in % 16 == 2; m = 136 > 128: a second stretch of the image; H = 12 larger than n = 5 and smaller
    # than n = 17 in one case; n = 130: a ragged third 64-column tile; out_mul alone
    C("cin130-k5", 130, 136, 5, 3, (5, 17, 130), (16, 32, 64), B=2, mul=math.sqrt(0.5)),
    # seven taps: a full and a ragged batch per block; tile 32 minus 1, 64 plus 1; out_div alone
    C("cin130-k7", 130, 40, 7, 1, (31, 65), (32, 64), div=3.0),
    # exactly eight taps (two full batches); tile 64 minus 1 and exact; tanh alone
    C("cin72-k8", 72, 24, 8, 1, (63, 64), (64, 64), post="tanh"),
    # H = 144, the cap, as k = 9, d = 18; nine taps: three batches per block, so the buffer parity alternates from block
    # to block over three blocks; n = 1 far below H, n = 150 above it; leaky_relu post-activation alone
    C("cin130-k9-H144", 130, 24, 9, 18, (1, 33, 150), (16, 64, 64), post="leaky_relu"),
    # H = 144 as k = 3, d = 72; leaky_relu pre-activation on exact zeros
    C("cin48-k3-H144", 48, 40, 3, 72, (16, 65), (16, 64), B=2, pre="leaky_relu"),
    # eleven taps on three blocks (parity alternates); everything together
    C("cin130-k11-all", 130, 40, 11, 1, (17, 64), (32, 64), B=2, pre="leaky_relu", post="tanh", **ALL),
    # eight blocks, the longest reduction (512 x 11); H = 20 above n = 9 and below n = 33
    C("cin512-k11", 512, 24, 11, 2, (9, 33), (16, 64), bias=True),
    # the wide 1 x 1 layer: eight blocks, H = 0, m = 136; relu pre-activation
    C("cin512-k1", 512, 136, 1, 1, (8, 130), (16, 64), pre="relu", bias=True),
    # one row of output over a full block; relu pre-activation on exact zeros; tile 32 exact
    C("cin64-cout1", 64, 1, 5, 3, (32,), (32,), B=3, pre="relu", bias=True),
    # m = m_pad = 128 over three blocks; tile 64 plus 1
    C("cin130-cout128", 130, 128, 3, 1, (65,), (64,), pre="leaky_relu", add1=True),
    # H = 0 on one full block with W = 16 and 32; tile 16 minus 1
    C("cin64-k1", 64, 40, 1, 1, (15, 32), (16, 32), B=3, add1=True, post="tanh"),
    # nine taps on a ragged second block (three batches in each: the parity differs between the two); one output row
    C("cin72-k9", 72, 1, 9, 2, (64,), (64,), B=3, bias=True),
    # everything together on the single-channel layer
    C("cin1-all", 1, 24, 3, 2, (1, 33), (16, 64), B=2, pre="leaky_relu", post="leaky_relu", **ALL),
    # ---- start of a stream (hist_in NULL)
    # zero padding; n = 1
    C("start-zero", 48, 24, 3, 1, (1, 17), (16, 32), B=2, start=True, bias=True),
    # replicate padding, also with a first chunk shorter than H = 12
    C("start-replicate", 72, 40, 5, 3, (1, 13, 40), (16, 16, 64), B=2, pad="replicate", start=True, pre="leaky_relu"),
    # reflect padding with a first chunk of exactly H + 1 columns, the shortest the check admits
    C("start-reflect", 72, 40, 5, 3, (13,), (16,), B=2, pad="reflect", start=True, pre="leaky_relu", bias=True),
    C("start-reflect-cin130", 130, 24, 7, 1, (7, 40), (16, 64), pad="reflect", start=True),
    # mid-stream under a reflect-padded descriptor: the history is read, the padding mode is not
    C("mid-reflect", 48, 24, 3, 2, (3, 20), (16, 32), B=2, pad="reflect", add1=True),
    C("mid-replicate", 48, 24, 3, 2, (3, 20), (16, 32), B=2, pad="replicate", mul=0.25),
    # ---- transposed, k = 2 s (H = 1, two taps)
    # m = 2: one row block, mostly padding; replicate start
    C("tr-4-2-1-start", 48, 1, 4, 1, (1, 17), (16, 32), B=2, s=2, pad="replicate", start=True),
    C("tr-4-2-1", 48, 1, 4, 1, (16, 33), (16, 64), B=3, s=2, pad="replicate", bias=True),
    # m = 96: phases of 24 rows, row blocks straddle them; zero start; add1 alone
    C("tr-8-4-24-start", 72, 24, 8, 1, (15, 64), (16, 64), s=4, start=True, add1=True),
    C("tr-8-4-24-all", 130, 24, 8, 1, (65,), (64,), B=2, s=4, pre="leaky_relu", post="tanh", **ALL),
    # m = 160 > 128: a row block straddles two phases (40 rows each) and the image's second stretch; ragged third tile
    C("tr-8-4-40", 64, 40, 8, 1, (17, 130), (32, 64), s=4, pad="replicate", div=3.0),
    C("tr-8-4-40-start", 130, 40, 8, 1, (1, 32), (16, 32), B=2, s=4, pad="replicate", start=True, pre="leaky_relu"),
    # m = 192 over eight blocks
    C("tr-16-8-24", 512, 24, 16, 1, (9,), (16,), s=8, pad="replicate", bias=True, add2=True, post="tanh"),
    C("tr-16-8-24-start", 1, 24, 16, 1, (33,), (64,), B=2, s=8, start=True, pre="relu"),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# the 32 x 64 tile: 8 (or, transposed, 8) row blocks x 2 column tiles x 32 items = 512 workgroups, the threshold
TILE_CASES = [C("tile-conv", 80, 256, 3, 1, (65,), (64,), B=32, bias=True, pre="leaky_relu"),
              C("tile-tr", 80, 32, 16, 1, (65,), (64,), B=32, s=8, pad="replicate", bias=True)]
# the layers of the delayed, slotted and mirrored forms: three staged blocks each
FORM_CONV = C("form-conv", 130, 40, 5, 3, (5, 33, 70, 12), (16, 64, 64, 16), B=2, pre="leaky_relu", bias=True, add1=True,
              add2=True, div=3.0, post="tanh")
FORM_TR = C("form-tr", 130, 24, 8, 1, (5, 33, 70, 12), (16, 64, 64, 16), B=2, s=4, pre="leaky_relu", bias=True, add1=True,
            add2=True, div=3.0, post="tanh")
MIRROR_CASES = [C("mirror-k7", 130, 40, 7, 1, (40,), (64,), B=2, pad="reflect", pre="leaky_relu", bias=True, post="tanh"),
                C("mirror-k3-d27", 130, 40, 3, 27, (70,), (64,), B=2, pad="reflect", pre="leaky_relu", bias=True)]
# the layers of the NaN-reach checks: the NaN sits in the last real channel of the third block
NAN_CONV = C("nan-conv", 130, 24, 5, 3, (40,), (64,), B=2, bias=True)
NAN_TR = C("nan-tr", 130, 24, 8, 1, (20,), (32,), B=2, s=4, bias=True)
EVERY_CASE = CASES + TILE_CASES + [FORM_CONV, FORM_TR] + MIRROR_CASES + [NAN_CONV, NAN_TR]
TWICE = ("cin130-k11-all", "tr-8-4-24-all")  # the plain cases that are launched twice


# ------------------------------------------------------------------------------------------------ inputs, shared
def hist_cols(c):
    return 1 if c.s else (c.k - 1) * c.d


def rate(c):
    return c.s or 1


Inputs = collections.namedtuple("Inputs", "x hist w bias add1 add2")


@functools.lru_cache(maxsize=None)
def inputs(c, n):
    """CPU float32 operands of one launch (read-only, shared): unit-variance data, weights scaled to a unit-variance
    contraction, so that no channel group, tap or history column is small against the largest output (the sensitivity
    check of tests/test_stream_refs_host.py).  With a pre-activation, exact zeros are planted in x and the history."""
    g = torch.Generator().manual_seed(7919 * EVERY_CASE.index(c) + n)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    H, t_out = hist_cols(c), n * rate(c)
    x = rn(c.B, c.cin, n)
    hist = rn(c.B, c.cin, H) if H and not c.start else None
    if c.pre:
        x[:, ::2, 1::3] = 0.0
        if hist is not None:
            hist[:, ::2, 1::3] = 0.0
    w = rn(c.cin, c.cout, c.k) / math.sqrt(2 * c.cin) if c.s else rn(c.cout, c.cin, c.k) / math.sqrt(c.cin * c.k)
    return Inputs(x, hist, w, rn(c.cout) if c.bias else None, rn(c.B, c.cout, t_out) if c.add1 else None,
                  rn(c.B, c.cout, t_out) if c.add2 else None)


def desc_of(c, n, B=None, pad=None):
    fused = dict(pre_act=c.pre, pre_slope=PRE_SLOPE if c.pre else 0.0, post_act=c.post,
                 post_slope=POST_SLOPE if c.post == "leaky_relu" else 0.0, out_mul=c.mul, out_div=c.div)
    B, pad = B or c.B, pad or c.pad
    if c.s:
        return ops.make_conv_desc(B, c.cin, c.cout, n, n * c.s, c.k, c.s, 1, c.s, 1, transposed=True, pad_mode=pad, **fused)
    return ops.make_conv_desc(B, c.cin, c.cout, n, n, c.k, 1, c.d, (c.k - 1) * c.d, 1, pad_mode=pad, **fused)


def _cast(t, dtype):
    return None if t is None else t.to(dtype)


def epilogue_of(c, t, dtype):
    return dict(bias=_cast(t.bias, dtype), out_mul=c.mul, out_div=c.div, post_act=c.post, post_slope=POST_SLOPE)


def contraction(c, win, w):
    if c.s:
        return R.contract_transposed(win, w, c.s, c.pre, PRE_SLOPE)
    return R.contract(win, w, c.d, c.pre, PRE_SLOPE)


def reference(c, t, dtype=torch.float64, w=None):
    """y of the plain launch of case ``c`` on the operands ``t``, by the rules of tests/stream_refs.py in ``dtype``."""
    win = R.window(_cast(t.hist, dtype), t.x.to(dtype), hist_cols(c), c.pad, bool(c.s))
    acc = contraction(c, win, (t.w if w is None else w).to(dtype))
    return R.epilogue(acc, add1=_cast(t.add1, dtype), add2=_cast(t.add2, dtype), **epilogue_of(c, t, dtype))


# ------------------------------------------------------------------------------------------------ launches
WORST = collections.defaultdict(float)


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for form, err in sorted(WORST.items()):
        print(f"worst rel-to-max error, {form}: {err:.3e} ({err / RTOL:.1%} of RTOL)")


def _within(got, want, form, what):
    assert torch.isfinite(got).all(), f"{what}: not finite"
    got = got.cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    err = (got - want).abs().max().item() / (want.abs().max().item() + 1e-12)
    WORST[form] = max(WORST[form], err)
    print(f"{what}: rel-to-max error {err:.3e}")
    assert err <= RTOL, f"{what}: rel-to-max error {err:.3e}"


def _image(device, c, t):
    """The fp32 packed image of the layer (it does not depend on the padding mode, which the packer admits as zero)."""
    return ops.pack_weight(desc_of(c, 16, B=1, pad="zero"), t.w.to(device))


def _dev(t, device, off=False):
    return None if t is None else _place(t, device, off)


def _guard(shape, device, off=0):
    return Guarded(shape, device, off) if math.prod(shape) else None


def _plain(device, c, n, t=None, off=False, B=None):
    """One plain launch -> (y, hist_out or None), both from guarded buffers.  ``off``: x, the addends and y start
    4 bytes off a 16-byte boundary."""
    t, B = t or inputs(c, n), B or c.B
    desc, H = desc_of(c, n, B), hist_cols(c)
    assert ops.conv1d_stream_supported(desc) and ops.conv1d_stream_hist_floats(desc) == B * c.cin * H
    what = f"{c.id} n{n} B{B} off={off}"
    with poison_lds():
        y = Guarded((B, c.cout, n * rate(c)), device, int(off))
        ho = _guard((B, c.cin, H), device)
        ops.conv1d_stream_forward(desc, _dev(t.x[:B], device, off), _dev(None if t.hist is None else t.hist[:B], device),
                                  ho.out if ho else None, _image(device, c, t), _dev(t.bias, device),
                                  _dev(None if t.add1 is None else t.add1[:B], device, off),
                                  _dev(None if t.add2 is None else t.add2[:B], device, off), out=y.out)
        return y.check(f"{what}: y"), ho.check(f"{what}: hist_out") if ho else None


def _check_history(c, t, got, what):
    H = hist_cols(c)
    if not H:
        assert got is None
        return
    want = R.history(t.hist, t.x, H, c.pad == "replicate")
    assert torch.equal(got.cpu(), want), f"{what}: hist_out differs from the last {H} columns of concat(hist_in, x)"


# ------------------------------------------------------------------------------------------------ the plain launch
@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_plain_chunk(c, device):
    for n, cols in zip(c.ns, c.tiles):
        assert ops.conv1d_stream_plan(desc_of(c, n))["tile"] == (16, cols)
        t = inputs(c, n)
        y, ho = _plain(device, c, n)
        _within(y, reference(c, t), "plain", f"{c.id} n{n}")
        _check_history(c, t, ho, f"{c.id} n{n}")
        if c.id in TWICE:
            y2, ho2 = _plain(device, c, n)
            assert torch.equal(y2, y) and torch.equal(ho2, ho), f"{c.id} n{n}: the second launch differs"


@pytest.mark.parametrize("cid", ["cin130-k11-all", "tr-8-4-24-all"])
def test_alignment(cid, device):
    """x, both addends and y 4 bytes off a 16-byte boundary: the same bits."""
    c = BY_ID[cid]
    for n in c.ns:
        y, ho = _plain(device, c, n)
        y4, ho4 = _plain(device, c, n, off=True)
        assert torch.equal(y4, y), f"{cid} n{n}: {int((y4 != y).sum())} values differ 4 bytes off"
        assert torch.equal(ho4, ho)


@pytest.mark.parametrize("c", TILE_CASES, ids=[c.id for c in TILE_CASES])
def test_32_row_tile(c, device):
    """512 workgroups of 32 x 64 at batch 32, against float64; the same input at batch 31 takes the 16 x 64 tile and
    gives the same bits for every shared item: the tile does not change an element's sum order."""
    n = c.ns[0]
    rows = c.cout * rate(c)
    assert ops.conv1d_stream_plan(desc_of(c, n)) == dict(tile=(32, 64), grid=(2, rows // 32, 32))
    assert ops.conv1d_stream_plan(desc_of(c, n, B=31)) == dict(tile=(16, 64), grid=(2, rows // 16, 31))
    t = inputs(c, n)
    y, ho = _plain(device, c, n)
    _within(y, reference(c, t), "plain, 32 x 64 tile", c.id)
    _check_history(c, t, ho, c.id)
    y31, ho31 = _plain(device, c, n, B=31)
    assert torch.equal(y31, y[:31]), f"{c.id}: {int((y31 != y[:31]).sum())} values differ between the tiles"
    assert torch.equal(ho31, ho[:31])


# ------------------------------------------------------------------------------------------------ NaN reach
def _nonfinite_columns(y):
    """The columns of item 0 that are non-finite -- in ALL rows, or the reach is not a column's -- item 1 being finite."""
    bad = ~torch.isfinite(y[0].cpu())
    assert torch.isfinite(y[1]).all(), "the NaN of item 0 reached item 1"
    cols = bad.any(0)
    assert torch.equal(bad.all(0), cols), "a column is non-finite in some rows only"
    return set(torch.nonzero(cols).flatten().tolist())


@pytest.mark.parametrize("where,col", [("x", 7), ("x", 39), ("hist", 0), ("hist", 4), ("hist", 11)])
def test_nan_reaches_exactly_its_taps(where, col, device):
    """One NaN in the last real channel of the last block, at chunk-relative column t (history column h: t = h - H): the
    non-finite output columns are exactly {t + i * d} inside the chunk.  No bound involved."""
    c, n = NAN_CONV, NAN_CONV.ns[0]
    t = inputs(c, n)
    x, hist = t.x.clone(), t.hist.clone()
    (x if where == "x" else hist)[0, c.cin - 1, col] = float("nan")
    y, _ = _plain(device, c, n, t._replace(x=x, hist=hist))
    at = col if where == "x" else col - hist_cols(c)
    assert _nonfinite_columns(y) == {at + i * c.d for i in range(c.k) if 0 <= at + i * c.d < n}


@pytest.mark.parametrize("where,col", [("x", 7), ("x", 19), ("hist", 0)])
def test_nan_reaches_exactly_its_two_taps_transposed(where, col, device):
    """... the 2 s output columns that x[j] (phases of column j) and x[j - 1] (phases of column j + 1) reach."""
    c, n = NAN_TR, NAN_TR.ns[0]
    t = inputs(c, n)
    x, hist = t.x.clone(), t.hist.clone()
    (x if where == "x" else hist)[0, c.cin - 1, col] = float("nan")
    y, _ = _plain(device, c, n, t._replace(x=x, hist=hist))
    at = col if where == "x" else -1
    assert _nonfinite_columns(y) == {j for j in range(at * c.s, (at + 2) * c.s) if 0 <= j < n * c.s}


# ------------------------------------------------------------------------------------------------ the delayed form
Lines = collections.namedtuple("Lines", "line1 line2")


@functools.lru_cache(maxsize=None)
def lines(c, n, delay1, delay2):
    """CPU float32 delay lines of a launch's two addends: inputs of the launch's own."""
    g = torch.Generator().manual_seed(104729 + 31 * n + delay1 + 7 * delay2 + EVERY_CASE.index(c))
    return Lines(*(torch.randn(c.B, c.cout, d, generator=g) if d else None for d in (delay1, delay2)))


# (n, delay1, delay2, window of the stride-1 layer, window of the transposed layer (t_out = 4 n), start of stream):
# delays 0, 1, 7 and 144, shorter and longer than n; windows full, empty, cut at either end, with an edge inside a tile
# and, transposed, edges that are no multiple of s
DELAYED = [
    (5, 0, 1, (0, 5), (0, 20), False),
    (5, 7, 144, (2, 4), (3, 18), False),
    (33, 7, 144, (9, 9), (50, 50), False),
    (33, 144, 7, (3, 30), (13, 101), False),
    (70, 1, 7, (0, 50), (0, 203), True),
    (70, 144, 0, (17, 70), (67, 280), False),
]


def _delayed_reference(c, t, ln, delay1, delay2, valid, dtype=torch.float64):
    win = R.window(_cast(t.hist, dtype), t.x.to(dtype), hist_cols(c), "zero", bool(c.s))
    return R.delayed_chunk(contraction(c, win, t.w.to(dtype)), valid, _cast(t.add1, dtype), _cast(ln.line1, dtype), delay1,
                           _cast(t.add2, dtype), _cast(ln.line2, dtype), delay2, **epilogue_of(c, t, dtype))


def _delayed(device, c, n, t, ln, delay1, delay2, valid):
    desc, H = desc_of(c, n), hist_cols(c)
    assert ops.conv1d_stream_delayed_supported(desc, delay1, delay2)
    what = f"{c.id} n{n} delays {delay1}, {delay2} valid {valid}"
    with poison_lds():
        y = Guarded((c.B, c.cout, n * rate(c)), device)
        ho = Guarded((c.B, c.cin, H), device)
        lo = [_guard((c.B, c.cout, d), device) for d in (delay1, delay2)]
        ops.conv1d_stream_delayed_forward(
            desc, _dev(t.x, device), _dev(t.hist, device), ho.out, _image(device, c, t), _dev(t.bias, device),
            _dev(t.add1, device), (_dev(ln.line1, device), lo[0].out if lo[0] else None), delay1,
            _dev(t.add2, device), (_dev(ln.line2, device), lo[1].out if lo[1] else None), delay2, valid, out=y.out)
        return (y.check(f"{what}: y"), ho.check(f"{what}: hist_out"),
                [g.check(f"{what}: line {i + 1}") if g else None for i, g in enumerate(lo)])


def _check_lines(got, adds, lines_in, delays, what):
    for i, (g, add, line, d) in enumerate(zip(got, adds, lines_in, delays)):
        if d:
            assert torch.equal(g.cpu(), R.line_out(line, add, d)), f"{what}: delay line {i + 1} is not the history rule's"
        else:
            assert g is None


@pytest.mark.parametrize("c", [FORM_CONV, FORM_TR], ids=["conv", "transposed"])
@pytest.mark.parametrize("n,delay1,delay2,valid_conv,valid_tr,start", DELAYED)
def test_delayed_form(c, n, delay1, delay2, valid_conv, valid_tr, start, device):
    valid = valid_tr if c.s else valid_conv
    t, ln = inputs(c, n), lines(c, n, delay1, delay2)
    if start:
        t, ln = t._replace(hist=None), Lines(None, None)
    y, ho, lo = _delayed(device, c, n, t, ln, delay1, delay2, valid)
    what = f"{c.id} n{n} delays {delay1}, {delay2}"
    want = _delayed_reference(c, t, ln, delay1, delay2, valid)
    _within(y, want, "delayed", what)
    outside = torch.cat([y[..., :valid[0]], y[..., valid[1]:]], -1)
    assert not outside.numel() or (outside.abs().max() == 0 and not torch.signbit(outside).any()), f"{what}: outside valid"
    _check_history(c, t, ho, what)
    _check_lines(lo, (t.add1, t.add2), ln, (delay1, delay2), what)
    if (n, delay1) == (33, 144):
        y2, ho2, lo2 = _delayed(device, c, n, t, ln, delay1, delay2, valid)
        assert torch.equal(y2, y) and torch.equal(ho2, ho) and all(torch.equal(a, b) for a, b in zip(lo2, lo))


# ------------------------------------------------------------------------------------------------ the slotted form
# per item (frames before, frames left, flags): a fresh one, a paused one, a running one
SLOT_ROWS = [(0, 9, ops.SLOT_LEFT_KNOWN), (3, 0, ops.SLOT_PAUSED), (5, 2, ops.SLOT_LEFT_KNOWN)]
SLOT_N, SLOT_DELAYS = 12, (3, 60)


@pytest.mark.parametrize("c,out_delay", [(FORM_CONV, 7), (FORM_TR, 10)], ids=["conv", "transposed"])
def test_slotted_form(c, out_delay, device):
    """A table with a fresh, a paused and a running item, against the references item by item: zeros-for-state for the
    fresh item (its state inputs are NaN-filled), state copy-through and zero output for the paused one (its x and
    addends are NaN-filled), the delayed form with the window rule's window for the running one."""
    n, (delay1, delay2), H, r = SLOT_N, SLOT_DELAYS, hist_cols(c), rate(c)
    t_out, w = n * r, inputs(c, n).w
    c = c._replace(B=3)
    g = torch.Generator().manual_seed(15485863 + r)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    t = Inputs(rn(3, c.cin, n), rn(3, c.cin, H), w, rn(c.cout), rn(3, c.cout, t_out), rn(3, c.cout, t_out))
    ln = Lines(rn(3, c.cout, delay1), rn(3, c.cout, delay2))
    nan = float("nan")
    dirty, dirty_ln = t._replace(x=t.x.clone(), hist=t.hist.clone(), add1=t.add1.clone(), add2=t.add2.clone()), \
        Lines(ln.line1.clone(), ln.line2.clone())
    for b, (before, _, flags) in enumerate(SLOT_ROWS):
        if before == 0:
            dirty.hist[b], dirty_ln.line1[b], dirty_ln.line2[b] = nan, nan, nan
        if flags & ops.SLOT_PAUSED:
            dirty.x[b], dirty.add1[b], dirty.add2[b] = nan, nan, nan
    desc = desc_of(c, n)

    def launch():
        with poison_lds():
            table = torch.tensor([row + (0,) for row in SLOT_ROWS], dtype=torch.int32, device=device)
            y, ho = Guarded((3, c.cout, t_out), device), Guarded((3, c.cin, H), device)
            lo = [Guarded((3, c.cout, d), device) for d in (delay1, delay2)]
            ops.conv1d_stream_slots_forward(
                desc, _dev(dirty.x, device), _dev(dirty.hist, device), ho.out, _image(device, c, t), _dev(t.bias, device),
                _dev(dirty.add1, device), (_dev(dirty_ln.line1, device), lo[0].out), delay1,
                _dev(dirty.add2, device), (_dev(dirty_ln.line2, device), lo[1].out), delay2,
                slots=table, rate=r, delay=out_delay, out=y.out)
            return y.check("y"), ho.check("hist_out"), [q.check("line") for q in lo]

    y, ho, lo = launch()
    for b, (before, left, flags) in enumerate(SLOT_ROWS):
        what = f"{c.id} item {b}"
        item = lambda v: v[b:b + 1]  # noqa: E731
        tb = Inputs(item(t.x), item(t.hist), t.w, t.bias, item(t.add1), item(t.add2))
        lb = Lines(item(ln.line1), item(ln.line2))
        if before == 0:
            tb, lb = tb._replace(hist=None), Lines(None, None)
        if flags & ops.SLOT_PAUSED:
            assert y[b].abs().max() == 0, f"{what}: a paused item's output is not zero"
            zeros = lambda v, like: torch.zeros_like(like) if v is None else v  # noqa: E731
            assert torch.equal(ho[b:b + 1].cpu(), zeros(tb.hist, item(t.hist))), f"{what}: history not copied through"
            for i, (got, line) in enumerate(zip(lo, lb)):
                assert torch.equal(got[b:b + 1].cpu(), zeros(line, item(ln[i]))), f"{what}: line {i + 1} not copied through"
            continue
        valid = R.slot_window(out_delay, r, t_out, before, left, bool(flags & ops.SLOT_LEFT_KNOWN))
        assert 0 < valid[0] or valid[1] < t_out, "the item's window cuts nothing"
        _within(item(y), _delayed_reference(c._replace(B=1), tb, lb, delay1, delay2, valid), "slotted", f"{what} valid {valid}")
        outside = torch.cat([y[b, :, :valid[0]], y[b, :, valid[1]:]], -1)
        assert outside.abs().max() == 0, f"{what}: outside valid"
        _check_history(c, tb, ho[b:b + 1], what)
        _check_lines([q[b:b + 1] for q in lo], (tb.add1, tb.add2), lb, (delay1, delay2), what)
    y2, ho2, lo2 = launch()
    assert torch.equal(y2, y) and torch.equal(ho2, ho) and all(torch.equal(a, b) for a, b in zip(lo2, lo))


# ------------------------------------------------------------------------------------------------ the mirrored form
# per layer the input windows (in_lo, in_hi): the left edge in the history and the right edge inside the chunk; the left
# edge alone; no edge in reach.  p = (k - 1) d / 2 = 3 and 27
MIRROR_WINDOWS = {"mirror-k7": [(-2, 30), (-4, None), (-2 ** 30, None), (3, 39)],
                  "mirror-k3-d27": [(-20, 60), (-40, None), (-2 ** 30, None), (-54, 69)]}


@pytest.mark.parametrize("c", MIRROR_CASES, ids=[c.id for c in MIRROR_CASES])
def test_mirrored_form(c, device):
    n, H = c.ns[0], hist_cols(c)
    p = H // 2
    t, desc = inputs(c, n), desc_of(c, n)
    assert ops.conv1d_stream_mirrored_supported(desc) and t.hist is not None
    for k, (in_lo, in_hi) in enumerate(MIRROR_WINDOWS[c.id]):
        valid = (max(in_lo + p, 0), n if in_hi is None else min(in_hi + p, n))

        def launch():
            with poison_lds():
                y, ho = Guarded((c.B, c.cout, n), device), Guarded((c.B, c.cin, H), device)
                ops.conv1d_stream_mirrored_forward(desc, _dev(t.x, device), _dev(t.hist, device), ho.out,
                                                   _image(device, c, t), _dev(t.bias, device), (in_lo, in_hi), valid, out=y.out)
                return y.check("y"), ho.check("hist_out")

        y, ho = launch()
        what = f"{c.id} input window ({in_lo}, {in_hi})"
        D = torch.float64
        win = R.mirror_window(t.hist.to(D), t.x.to(D), H, in_lo, in_hi)
        want = R.zero_outside(R.epilogue(contraction(c, win, t.w.to(D)), **epilogue_of(c, t, D)), *valid)
        _within(y, want, "mirrored", what)
        outside = torch.cat([y[..., :valid[0]], y[..., valid[1]:]], -1)
        assert not outside.numel() or outside.abs().max() == 0, f"{what}: outside valid"
        assert torch.equal(ho.cpu(), R.history(t.hist, t.x, H)), f"{what}: the history is not raw"
        if k == 0:
            y2, ho2 = launch()
            assert torch.equal(y2, y) and torch.equal(ho2, ho)
