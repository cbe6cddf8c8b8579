"""GPU: the HiFi-GAN V1 generator with its 32- / 64-channel residual units routed to the split-operand unit
(csrc/resunit_split.hip).  The admission tables are forced to "everything supported"
(``_ConvNd.split_admit_all``), so that the short test inputs reach the kernel on every unit; the last test runs single
blocks under the default table at its shortest admitted length."""
import pytest
import torch

from oracle import torch_cpu
from parallelwavegan_amd import ops
from parallelwavegan_amd.graphs import GraphedInference
from parallelwavegan_amd.layers.conv import _ConvNd
from parallelwavegan_amd.models import HiFiGANGenerator
from tests.golden import synth
from tests.util import WAVE_TOL, max_abs, synth_for

pytestmark = pytest.mark.gpu

UNIT_SPLIT = "resunit_split_kernel"
UNIT_FP32 = "resunit_kernel"
CONV_SPLIT = "conv1d_split_mfma_kernel"


@pytest.fixture
def admit_all(monkeypatch):
    monkeypatch.setattr(_ConvNd, "split_exact", True)
    monkeypatch.setattr(_ConvNd, "split_admit_all", True)


def _v1(device, seed=5):
    g = HiFiGANGenerator(**synth.HIFIGAN_V1)
    sd = synth_for(g, seed, 1.25)
    g.load_state_dict(sd)
    return g.to(device).eval(), sd


@pytest.mark.parametrize("batch,frames", [(2, 24), (1, 40)])
def test_generator_matches_oracle_and_switch_off_is_the_default_path(batch, frames, admit_all, device):
    g, sd = _v1(device)
    c = synth.synth_input("c", (batch, 80, frames), seed=frames)
    with torch.no_grad():
        ref = torch_cpu.hifigan_generator(sd, c, **synth.HIFIGAN_V1)
        with ops.profile() as prof:
            y = g(c.to(device)).clone()
        assert UNIT_SPLIT in prof.results and UNIT_FP32 not in prof.results, sorted(prof.results)
        # 2 stages x 3 kernel sizes x 3 dilations, the 64-channel k = 11 class included
        assert prof.results[UNIT_SPLIT]["launches"] == 18, prof.results[UNIT_SPLIT]
        _ConvNd.split_exact = False
        with ops.profile() as prof_off:
            y_off = g(c.to(device)).clone()
        assert UNIT_SPLIT not in prof_off.results and UNIT_FP32 in prof_off.results
        _ConvNd.split_admit_all = False  # the admission tables themselves admit no launch this short
        _ConvNd.split_exact = True
        with ops.profile() as prof_dflt:
            y_dflt = g(c.to(device)).clone()
        assert UNIT_SPLIT not in prof_dflt.results and UNIT_FP32 in prof_dflt.results
    print(f"max abs vs oracle: split units {max_abs(y, ref):.3e}, fp32 kernels {max_abs(y_off, ref):.3e}")
    assert y.shape == ref.shape
    assert max_abs(y, ref) <= WAVE_TOL
    assert max_abs(y_off, ref) <= WAVE_TOL
    assert torch.equal(y_off, y_dflt), "the switch turned off must leave exactly the default path"
    assert not torch.equal(y, y_off), "different kernels: equal bits mean the split units did not run"


def test_chained_forked_and_serial_are_bit_identical(admit_all, device):
    """The MRF forms of tests/test_hifigan_split_gpu.py on a generator whose two stages are 64 and 32 channels wide:
    every unit is a split unit; eager and captured (branches fork only inside a capture)."""
    torch.manual_seed(3)
    g = HiFiGANGenerator(channels=128, upsample_scales=(4, 4), upsample_kernel_sizes=(8, 8)).to(device).eval()
    c = torch.randn(2, 80, 40, device=device)
    with torch.no_grad():
        with ops.profile() as prof:
            serial = g(c).clone()
        assert UNIT_SPLIT in prof.results and UNIT_FP32 not in prof.results, sorted(prof.results)
        g.branch_streams = True
        g.chain_min_elems = 0
        chained = g(c).clone()
        chained_graph = GraphedInference(g)(c).clone()
        g.chain_min_elems = 1 << 62
        forked = g(c).clone()
        forked_graph = GraphedInference(g)(c).clone()
    torch.cuda.synchronize()
    for y in (chained, chained_graph, forked, forked_graph):
        assert torch.equal(y, serial)


def test_graph_replay_equals_eager_and_follows_the_switch(admit_all, device):
    g, _ = _v1(device)
    c = synth.synth_input("c", (2, 80, 24), seed=24).to(device)
    with torch.no_grad():
        e_on = g(c).clone()
        run = GraphedInference(g)
        assert torch.equal(run(c), e_on)
        graph_on = run._graphs[next(iter(run._graphs))][0]
        assert torch.equal(run(c), e_on) and run._graphs[next(iter(run._graphs))][0] is graph_on
        _ConvNd.split_exact = False
        e_off = g(c).clone()
        r_off = run(c).clone()  # the switch is part of the compared state: the graph of the split launches is dropped
        assert run._graphs[next(iter(run._graphs))][0] is not graph_on
        assert torch.equal(r_off, e_off) and not torch.equal(r_off, e_on)
        _ConvNd.split_exact = True
        assert torch.equal(run(c), e_on)


def test_a_forward_that_needs_gradients_launches_neither_split_kernel(admit_all, device):
    g, _ = _v1(device)
    c = synth.synth_input("c", (1, 80, 24), seed=3).to(device)

    def none_of(prof):
        return UNIT_SPLIT not in prof.results and CONV_SPLIT not in prof.results

    with ops.profile() as prof:
        y = g(c)  # parameters require grad
    assert y.requires_grad and none_of(prof), sorted(prof.results)
    for p in g.parameters():
        p.requires_grad_(False)
    with ops.profile() as prof:
        y = g(c.clone().requires_grad_())  # only the input does
    assert y.requires_grad and none_of(prof), sorted(prof.results)
    with ops.profile() as prof:
        g(c)  # nothing does: the inference path, grad mode on or off
    assert UNIT_SPLIT in prof.results and CONV_SPLIT in prof.results


@pytest.mark.parametrize("channels,kernel,form_kernel", [(64, 7, CONV_SPLIT), (64, 3, UNIT_SPLIT), (32, 11, UNIT_SPLIT),
                                                          (32, 3, UNIT_FP32)])
def test_default_table_routes_a_block_and_both_forms_give_the_same_bits(channels, kernel, form_kernel, monkeypatch,
                                                                        device):
    """Under the default table, at the shortest admitted length (2 x 12800 columns): the listed form runs alone (the
    pair of general split launches at C = 64, k = 7; the one-launch unit at C = 64, k = 3 and C = 32, k = 11; the fp32
    unit at C = 32, k = 3, which is not listed), and the forced one-launch unit gives the bits of the pair."""
    from parallelwavegan_amd.layers import HiFiGANResidualBlock

    monkeypatch.setattr(_ConvNd, "split_exact", True)
    monkeypatch.setattr(_ConvNd, "split_admit_all", False)
    torch.manual_seed(channels + kernel)
    blk = HiFiGANResidualBlock(kernel, channels, (1, 3, 5)).to(device)
    x = torch.randn(2, channels, 12800, device=device)
    accum = torch.randn_like(x)
    with torch.no_grad():
        with ops.profile() as prof:
            y = blk(x, accum=accum, out_div=3.0).clone()
        assert sorted(prof.results) == [form_kernel], sorted(prof.results)
        assert prof.results[form_kernel]["launches"] == (6 if form_kernel == CONV_SPLIT else 3)
        short = blk(x[:, :, :8192].contiguous())  # 16384 columns: under the floor, the fp32 path
        _ConvNd.split_exact = False
        assert torch.equal(blk(x[:, :, :8192].contiguous()), short)
        _ConvNd.split_exact = True
        _ConvNd.split_admit_all = True
        with ops.profile() as prof_all:
            y_unit = blk(x, accum=accum, out_div=3.0)
        assert sorted(prof_all.results) == [UNIT_SPLIT]
    if form_kernel == UNIT_FP32:
        assert not torch.equal(y, y_unit) and max_abs(y, y_unit) <= 3e-5 * float(y.abs().max())  # the fp32 bar
    else:
        assert torch.equal(y, y_unit), "the unit kernel and the pair of split launches are one definition"
