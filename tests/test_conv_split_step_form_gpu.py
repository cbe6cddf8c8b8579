"""GPU: the two forms of the split-operand kernel's reduction step (csrc/conv1d_split.hip) through
``pwg_conv1d_split_forward_step``: ``conv1d_split_mfma_kernel`` (resident) and ``conv1d_split_streamed_mfma_kernel``
(the weight fragments requested a row tile ahead of their MFMAs, across taps and chunks) issue the same products in the
same order, so they must give the same bits -- as each other, at full-size and half-size tiles, and on a repeated
launch -- and stay within 3e-5 of the largest output of the float64 convolution (RTOL of tests/test_conv_split_gpu.py).

Shapes: those of tests/test_split_prefetch_gpu.py (one step in total, a chunk crossing per step, taps and chunks
dilated, 1 / 2 / 4 row tiles per wave with padded rows), and 256 -> 256, k = 3, T = 132: eight chunks (the prefetch
crosses seven chunk stagings), two row blocks.  Batch 2, both MFMA shapes, ``torch.randn`` inputs with fixed seeds,
poisoned LDS, poisoned and guarded outputs."""
import functools

import pytest
import torch
import torch.nn.functional as F

from parallelwavegan_amd import ops
from tests.test_conv_split_gpu import RTOL, Guarded
from tests.test_split_prefetch_gpu import CONV_CASES as PREFETCH_CASES
from tests.util import poison_empty, poison_lds

pytestmark = pytest.mark.gpu

B = 2
# name -> c_in, c_out, T, k, dilation
CASES = dict(PREFETCH_CASES, eight_chunks_two_row_blocks=(256, 256, 132, 3, 1))
RESIDENT, STREAMED = 1, 2


@functools.lru_cache(maxsize=None)
def _inputs(name):
    cin, cout, t, k, _ = CASES[name]
    g = torch.Generator().manual_seed(77000 + sorted(CASES).index(name))
    return torch.randn(B, cin, t, generator=g), torch.randn(cout, cin, k, generator=g) / (cin * k) ** 0.5


@functools.lru_cache(maxsize=None)
def _ref(name):
    """The 'same' convolution in float64 from the fp32 operands, as k matrix products over shifted views."""
    _, cout, t, k, dil = CASES[name]
    x, w = _inputs(name)
    pad = (k - 1) // 2 * dil
    xp = F.pad(x.double(), (pad, pad))
    y = torch.zeros(B, cout, t, dtype=torch.float64)
    for tap in range(k):
        y += torch.matmul(w[:, :, tap].double(), xp[:, :, tap * dil:tap * dil + t])
    return y


@pytest.mark.parametrize("mfma_shape", [16, 32])
@pytest.mark.parametrize("name", list(CASES))
def test_step_forms_agree(name, mfma_shape, device):
    cin, cout, t, k, dil = CASES[name]
    x, w = (v.to(device) for v in _inputs(name))
    ref = _ref(name).to(device)
    scale = float(ref.abs().max())
    desc = ops.make_conv_desc(B, cin, cout, t, t, k, 1, dil, (k - 1) // 2 * dil)
    assert ops.conv1d_split_supported(desc)

    def launch(tile_mode, step_form):
        gd = Guarded((B, cout, t), device)
        ops.conv1d_forward_split(desc, x, ws, out=gd.out, mfma_shape=mfma_shape, tile_mode=tile_mode, step_form=step_form)
        return gd.check(f"{name} {mfma_shape} tile_mode {tile_mode} step_form {step_form}")

    with poison_lds(), poison_empty():
        ws = ops.pack_weight_split(desc, w)
        res = {tm: launch(tm, RESIDENT) for tm in (1, 2)}
        stm = {tm: launch(tm, STREAMED) for tm in (1, 2)}
        again = launch(1, STREAMED)
        planned = ops.conv1d_forward_split(desc, x, ws, mfma_shape=mfma_shape)
    for tm in (1, 2):
        err = float((stm[tm].double() - ref).abs().max()) / scale
        print(f"{name} {mfma_shape} tile_mode {tm}: streamed rel-to-max error {err:.3e}")
        assert err <= RTOL, f"tile_mode {tm}: rel-to-max error {err:.3e}"
        assert torch.equal(stm[tm], res[tm]), f"tile_mode {tm}: the streamed and the resident form differ"
    assert torch.equal(stm[1], stm[2]), "streamed: the two tile modes differ"
    assert torch.equal(res[1], res[2]), "resident: the two tile modes differ"
    assert torch.equal(stm[1], again), "two streamed launches on the same inputs differ"
    assert torch.equal(stm[1], planned), "the plan's own launch differs"


def test_step_form_out_of_range_launches_nothing(device):
    cin, cout, t, k, dil = CASES["one_step"]
    x, w = (v.to(device) for v in _inputs("one_step"))
    desc = ops.make_conv_desc(B, cin, cout, t, t, k, 1, dil, 0)
    ws = ops.pack_weight_split(desc, w)
    out = torch.full((B, cout, t), float("nan"), device=device)
    for bad in (3, -1):
        with pytest.raises(RuntimeError, match="step_form"):
            ops.conv1d_forward_split(desc, x, ws, out=out, step_form=bad)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
