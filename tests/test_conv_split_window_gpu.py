"""GPU: the two forms of the split-operand kernel's window staging (csrc/conv1d_split.hip) through
``pwg_conv1d_split_forward_window``: ``conv1d_split_mfma_kernel`` (staged) and ``conv1d_split_window_mfma_kernel`` (the
raw fp32 window of chunk n + 1 requested by LDS-DMA in front of the tap loop of chunk n and split behind it) write the
same values to the same plane addresses, so they must give the same bits -- as each other, at full-size and half-size
tiles, on a repeated launch and from the plan's own launch -- and stay within 3e-5 of the largest output of the float64
convolution (RTOL of tests/test_conv_split_gpu.py).

Shapes, the smallest at which the prefetched kernel can go wrong:
  64 -> 64, k = 3, d = 5, T = 404    edge, interior, interior and edge tiles at the full-size tile; two chunks: one
                                     prefetch crossing
  96 -> 72, k = 3, d = 1, T = 404    three chunks: the raw region is reused twice; padded rows
  80 -> 64, k = 7, d = 5, T = 404    prefetched chunks followed by a checked 16-channel tail chunk
  256 -> 256, k = 3, T = 132         eight chunks, two row blocks, no interior tile at the full-size tile: the kernel
                                     never prefetches there
  64 -> 64, k = 1, T = 640           no halo: the window is exactly the tile
  T = 402                            not a multiple of 4: no 16-B staging; the plan answers staged, a forced 2 is refused
  one case with every epilogue term  bias, add1, add2 = y, out_div = 3, tanh, and a leaky pre-activation
Batch 2 with different data per item (a prefetch that ran past an item's row would show), both MFMA shapes,
``torch.randn`` inputs with fixed seeds, poisoned LDS, poisoned and guarded outputs."""
import functools

import pytest
import torch
import torch.nn.functional as F

from parallelwavegan_amd import ops
from tests.test_conv_split_gpu import RTOL, Guarded
from tests.util import poison_empty, poison_lds

pytestmark = pytest.mark.gpu

B = 2
# name -> c_in, c_out, T, k, dilation
CASES = {
    "two_chunks_edge_interior": (64, 64, 404, 3, 5),
    "three_chunks_padded_rows": (96, 72, 404, 3, 1),
    "tail_chunk_after_prefetched": (80, 64, 404, 7, 5),
    "eight_chunks_no_interior": (256, 256, 132, 3, 1),
    "no_halo": (64, 64, 640, 1, 1),
}
STAGED, PREFETCHED = 1, 2
SLOPE = 0.1


@functools.lru_cache(maxsize=None)
def _inputs(name):
    cin, cout, t, k, _ = CASES[name]
    g = torch.Generator().manual_seed(88000 + sorted(CASES).index(name))
    return dict(x=torch.randn(B, cin, t, generator=g), w=torch.randn(cout, cin, k, generator=g) / (cin * k) ** 0.5,
                bias=torch.randn(cout, generator=g), add1=torch.randn(B, cout, t, generator=g),
                add2=torch.randn(B, cout, t, generator=g))


@functools.lru_cache(maxsize=None)
def _conv64(name, activated):
    """The 'same' convolution in float64 from the fp32 operands, as k matrix products over shifted views; the leaky
    pre-activation is applied in fp32, as the kernels define it."""
    _, cout, t, k, dil = CASES[name]
    v = _inputs(name)
    x = F.leaky_relu(v["x"], SLOPE) if activated else v["x"]
    pad = (k - 1) // 2 * dil
    xp = F.pad(x.double(), (pad, pad))
    y = torch.zeros(B, cout, t, dtype=torch.float64)
    for tap in range(k):
        y += torch.matmul(v["w"][:, :, tap].double(), xp[:, :, tap * dil:tap * dil + t])
    return y


@pytest.mark.parametrize("mfma_shape", [16, 32])
@pytest.mark.parametrize("name", list(CASES))
def test_window_forms_agree(name, mfma_shape, device):
    cin, cout, t, k, dil = CASES[name]
    v = _inputs(name)
    x, w = v["x"].to(device), v["w"].to(device)
    ref = _conv64(name, False).to(device)
    scale = float(ref.abs().max())
    desc = ops.make_conv_desc(B, cin, cout, t, t, k, 1, dil, (k - 1) // 2 * dil)
    assert ops.conv1d_split_supported(desc)

    def launch(tile_mode, window_form):
        gd = Guarded((B, cout, t), device)
        ops.conv1d_forward_split(desc, x, ws, out=gd.out, mfma_shape=mfma_shape, tile_mode=tile_mode,
                                 window_form=window_form)
        return gd.check(f"{name} {mfma_shape} tile_mode {tile_mode} window_form {window_form}")

    with poison_lds(), poison_empty():
        ws = ops.pack_weight_split(desc, w)
        stg = {tm: launch(tm, STAGED) for tm in (1, 2)}
        pre = {tm: launch(tm, PREFETCHED) for tm in (1, 2)}
        again = launch(1, PREFETCHED)
        planned = ops.conv1d_forward_split(desc, x, ws, mfma_shape=mfma_shape)
    for tm in (1, 2):
        err = float((pre[tm].double() - ref).abs().max()) / scale
        print(f"{name} {mfma_shape} tile_mode {tm}: prefetched rel-to-max error {err:.3e}")
        assert err <= RTOL, f"tile_mode {tm}: rel-to-max error {err:.3e}"
        assert torch.equal(pre[tm], stg[tm]), f"tile_mode {tm}: the prefetched and the staged form differ"
    assert torch.equal(pre[1], pre[2]), "prefetched: the two tile modes differ"
    assert torch.equal(stg[1], stg[2]), "staged: the two tile modes differ"
    assert torch.equal(pre[1], again), "two prefetched launches on the same inputs differ"
    assert torch.equal(pre[1], planned), "the plan's own launch differs"


@pytest.mark.parametrize("mfma_shape", [16, 32])
def test_every_epilogue_term(mfma_shape, device):
    """bias, add1, add2 = y (in place), out_div = 3, tanh and a leaky pre-activation, on the case with edge and interior
    tiles."""
    name = "two_chunks_edge_interior"
    cin, cout, t, k, dil = CASES[name]
    v = {n: a.to(device) for n, a in _inputs(name).items()}
    ref = torch.tanh((_conv64(name, True) + _inputs(name)["bias"].double().view(1, -1, 1) + _inputs(name)["add1"].double()
                      + _inputs(name)["add2"].double()) / 3.0).to(device)
    desc = ops.make_conv_desc(B, cin, cout, t, t, k, 1, dil, (k - 1) // 2 * dil, pre_act="leaky_relu", pre_slope=SLOPE,
                              post_act="tanh", out_div=3.0)

    def launch(tile_mode, window_form):
        gd = Guarded((B, cout, t), device)
        gd.out.copy_(v["add2"])
        ops.conv1d_forward_split(desc, v["x"], ws, v["bias"], v["add1"], gd.out, out=gd.out, mfma_shape=mfma_shape,
                                 tile_mode=tile_mode, window_form=window_form)
        return gd.check(f"epilogue {mfma_shape} tile_mode {tile_mode} window_form {window_form}")

    with poison_lds(), poison_empty():
        ws = ops.pack_weight_split(desc, v["w"])
        stg = {tm: launch(tm, STAGED) for tm in (1, 2)}
        pre = {tm: launch(tm, PREFETCHED) for tm in (1, 2)}
    for tm in (1, 2):
        err = float((pre[tm].double() - ref).abs().max()) / float(ref.abs().max())
        print(f"epilogue {mfma_shape} tile_mode {tm}: prefetched rel-to-max error {err:.3e}")
        assert err <= RTOL, f"tile_mode {tm}: rel-to-max error {err:.3e}"
        assert torch.equal(pre[tm], stg[tm]), f"tile_mode {tm}: the prefetched and the staged form differ"
    assert torch.equal(pre[1], pre[2]), "prefetched: the two tile modes differ"


def test_no_16_byte_staging_is_staged_and_a_forced_prefetch_launches_nothing(device):
    """T = 402 is not a multiple of 4: the plan answers staged and a forced 2 is refused; so are a window_form out of
    range and the streamed step named together with the prefetched window."""
    cin, cout, t, k, dil = 64, 64, 402, 3, 5
    g = torch.Generator().manual_seed(88100)
    x = torch.randn(B, cin, t, generator=g).to(device)
    w = (torch.randn(cout, cin, k, generator=g) / (cin * k) ** 0.5).to(device)
    desc = ops.make_conv_desc(B, cin, cout, t, t, k, 1, dil, dil)
    assert ops.conv1d_split_window_form(desc) == "staged"
    ws = ops.pack_weight_split(desc, w)
    out = torch.full((B, cout, t), float("nan"), device=device)
    with pytest.raises(RuntimeError, match="16-B staging"):
        ops.conv1d_forward_split(desc, x, ws, out=out, window_form=PREFETCHED)
    for bad in (3, -1):
        with pytest.raises(RuntimeError, match="window_form"):
            ops.conv1d_forward_split(desc, x, ws, out=out, window_form=bad)
    ok = ops.make_conv_desc(B, cin, cout, 404, 404, k, 1, dil, dil)
    x4, out4 = torch.randn(B, cin, 404, device=device), torch.full((B, cout, 404), float("nan"), device=device)
    with pytest.raises(RuntimeError, match="streamed"):
        ops.conv1d_forward_split(ok, x4, ws, out=out4, step_form=2, window_form=PREFETCHED)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(out4).all())
    # the staged form of the same launch is untouched by the refusals
    y = ops.conv1d_forward_split(desc, x, ws, window_form=STAGED)
    assert torch.equal(y, ops.conv1d_forward_split(desc, x, ws))
