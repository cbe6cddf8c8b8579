"""GPU: a HiFi-GAN generator whose last two stages are 64 and 32 channels wide, with the k = 3 residual blocks of those
stages run as ONE launch each (resblock_split_kernel of csrc/resunit_split.hip; DESIGN.md s9.2, "The chained block")
under the DEFAULT tables, at the shortest length that reaches every row of ``RESBLOCK_SPLIT_ADMITTED``.  The block is
defined as the chain of unit launches it replaces, so the forward with the rows on equals the forward with them off to
the bit: eager, with chained MRF branches, and under ``GraphedInference``."""
import pytest
import torch

from parallelwavegan_amd import ops
from parallelwavegan_amd.graphs import GraphedInference
from parallelwavegan_amd.layers import HiFiGANResidualBlock
from parallelwavegan_amd.layers import conv as conv_mod
from parallelwavegan_amd.layers.conv import _ConvNd
from parallelwavegan_amd.models import HiFiGANGenerator

pytestmark = pytest.mark.gpu

BLOCK, UNIT_SPLIT = "resblock_split_kernel", "resunit_split_kernel"
BATCH = 2


def _frames():
    """Mel frames at which both stages (64 channels at 4 columns per frame, 32 at 16) reach their rows' floors."""
    table = conv_mod.RESBLOCK_SPLIT_ADMITTED
    assert set(table) == {(32, 3), (64, 3)}, "this test covers the rows it knows: " + str(sorted(table))
    need = max(-(-table[(64, 3)][1] // (BATCH * 4)), -(-table[(32, 3)][1] // (BATCH * 16)))
    return (need + 3) // 4 * 4


@pytest.fixture
def generator(monkeypatch, device):
    monkeypatch.setattr(_ConvNd, "split_exact", True)
    monkeypatch.setattr(_ConvNd, "split_admit_all", False)
    monkeypatch.setattr(HiFiGANResidualBlock, "fuse_block", True)
    torch.manual_seed(3)
    g = HiFiGANGenerator(channels=128, upsample_scales=(4, 4), upsample_kernel_sizes=(8, 8)).to(device).eval()
    for p in g.parameters():
        p.requires_grad_(False)
    return g, torch.randn(BATCH, 80, _frames(), device=device)


def _launches(prof, name):
    return prof.results[name]["launches"] if name in prof.results else 0


def test_rows_on_equal_rows_off_eager(generator, device):
    g, c = generator
    with torch.no_grad():
        with ops.profile() as prof_on:
            on = g(c).clone()
        # the k = 3 block of each of the two stages is one launch; the k = 7 / 11 blocks stay on their units and pairs
        assert _launches(prof_on, BLOCK) == 2, sorted(prof_on.results)
        HiFiGANResidualBlock.fuse_block = False
        with ops.profile() as prof_off:
            off = g(c).clone()
        assert _launches(prof_off, BLOCK) == 0
        assert _launches(prof_off, UNIT_SPLIT) == _launches(prof_on, UNIT_SPLIT) + 6
        assert torch.equal(on, off), "the block is the chain of its units"
        # the split switch off: the parent's path and bits, no block
        HiFiGANResidualBlock.fuse_block = True
        _ConvNd.split_exact = False
        with ops.profile() as prof_exact_off:
            fp32 = g(c).clone()
        HiFiGANResidualBlock.fuse_block = False
        assert _launches(prof_exact_off, BLOCK) == 0 and torch.equal(g(c), fp32)


def test_graph_replay_equals_eager_and_follows_the_switch(generator, device):
    """Inside the capture the MRF blocks run as chained branches (they fork only there): the first branch's join waits
    for nothing, so the k = 3 block is one launch there too; the k = 7 / 11 branches keep their join in front of their
    last kernel."""
    g, c = generator
    g.branch_streams = True
    g.chain_min_elems = 0
    with torch.no_grad():
        eager = g(c).clone()
        run = GraphedInference(g)
        assert torch.equal(run(c), eager)
        graph_on = run._graphs[next(iter(run._graphs))][0]
        assert torch.equal(run(c), eager) and run._graphs[next(iter(run._graphs))][0] is graph_on
        HiFiGANResidualBlock.fuse_block = False
        r_off = run(c).clone()  # the switch is part of the compared state: the graph with the block launches is dropped
        assert run._graphs[next(iter(run._graphs))][0] is not graph_on
        assert torch.equal(r_off, eager) and torch.equal(g(c), eager)


def test_a_forward_that_needs_gradients_launches_no_block(generator, device):
    g, c = generator
    with ops.profile() as prof:
        y = g(c.clone().requires_grad_())
    assert y.requires_grad and _launches(prof, BLOCK) == 0, sorted(prof.results)
