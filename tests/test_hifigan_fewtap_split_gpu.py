"""GPU: the k = 3 residual blocks of the HiFi-GAN V1 generator routed to the split-operand kernels -- the 128-channel
convolutions by the few-tap admission table (``layers/conv.py``, ``SPLIT_FEWTAP_ADMITTED``), the
32-channel units by their row of ``RESUNIT_SPLIT_ADMITTED`` (s9.2) -- under the DEFAULT tables, at the table's floor."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from parallelwavegan_amd import ops
from parallelwavegan_amd.layers import HiFiGANResidualBlock
from parallelwavegan_amd.layers import conv as conv_mod
from parallelwavegan_amd.layers.conv import _ConvNd
from tests.util import max_abs

pytestmark = pytest.mark.gpu

CONV_SPLIT, UNIT_SPLIT = "conv1d_split_mfma_kernel", "resunit_split_kernel"
KERNEL, DILATIONS, SLOPE = 3, (1, 3, 5), 0.1
# channels -> the kernel that runs the block alone at the floor, its launches, the table and the key of the class
CLASSES = {
    128: (CONV_SPLIT, 6, "SPLIT_FEWTAP_ADMITTED", (128, 128, KERNEL)),
    32: (UNIT_SPLIT, 3, "RESUNIT_SPLIT_ADMITTED", (32, KERNEL, True)),
}
RTOL = 3e-5  # the fp32 bar of tests/test_hifigan_resunit_split_gpu.py, of the largest magnitude


@functools.lru_cache(maxsize=None)
def _block_and_input(channels):
    """The block (CPU, fp32) and an input of 2 x floor / 2 columns, shared by the tests (read-only)."""
    _, _, table, key = CLASSES[channels]
    floor = getattr(conv_mod, table)[key]
    floor = floor[1] if isinstance(floor, tuple) else floor
    assert floor % 8 == 0
    torch.manual_seed(channels + KERNEL)
    blk = HiFiGANResidualBlock(KERNEL, channels, DILATIONS).eval()
    for p in blk.parameters():
        p.requires_grad_(False)
    return blk, torch.randn(2, channels, floor // 2)


@functools.lru_cache(maxsize=None)
def _ref64(channels):
    """The block in float64 from its fp32 parameters; the activations are applied in fp32 to fp32 inputs by the kernels,
    here to the float64 intermediate (the difference is an ulp of fp32 per activation, far under the bar)."""
    blk, x = _block_and_input(channels)
    y = x.double()
    for i, d in enumerate(DILATIONS):
        c1, c2 = blk.convs1[i][1], blk.convs2[i][1]
        h = F.conv1d(F.leaky_relu(y, SLOPE), c1.weight.double(), c1.bias.double(), padding=d, dilation=d)
        y = y + F.conv1d(F.leaky_relu(h, SLOPE), c2.weight.double(), c2.bias.double(), padding=1)
    return y


@pytest.mark.parametrize("channels", list(CLASSES))
def test_default_table_routes_the_block_at_its_floor(channels, monkeypatch, device):
    split_kernel, launches, table, _ = CLASSES[channels]
    monkeypatch.setattr(_ConvNd, "split_exact", True)
    monkeypatch.setattr(_ConvNd, "split_admit_all", False)
    ref = _ref64(channels).to(device)
    blk, x = _block_and_input(channels)
    blk, x = copy.deepcopy(blk).to(device), x.to(device)
    with torch.no_grad():
        with ops.profile() as prof:
            y = blk(x).clone()
        assert sorted(prof.results) == [split_kernel], sorted(prof.results)
        assert prof.results[split_kernel]["launches"] == launches, prof.results[split_kernel]
        # one 4-column step under the floor: the fp32 path, whatever the switch says
        short = x[:, :, :-2].contiguous()
        with ops.profile() as prof_short:
            y_short = blk(short).clone()
        assert split_kernel not in prof_short.results, sorted(prof_short.results)
        _ConvNd.split_exact = False
        assert torch.equal(blk(short), y_short)
        # the switch off at the floor: the fp32 path's bits, those the block gives with an empty table
        with ops.profile() as prof_off:
            y_off = blk(x).clone()
        assert split_kernel not in prof_off.results, sorted(prof_off.results)
        _ConvNd.split_exact = True
        monkeypatch.setattr(conv_mod, table, {})
        assert torch.equal(blk(x), y_off)
    assert not torch.equal(y, y_off), "the two paths are different kernels: equal bits mean the split path did not run"
    scale = float(ref.abs().max())
    err, err_off = max_abs(y.double(), ref) / scale, max_abs(y_off.double(), ref) / scale
    print(f"block {channels} k{KERNEL} at 2 x {x.shape[2]} columns: rel-to-max error split {err:.3e}, fp32 kernels {err_off:.3e}")
    assert err <= RTOL and err_off <= RTOL
