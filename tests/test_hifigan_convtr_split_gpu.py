"""GPU: the HiFi-GAN V1 generator with its four upsampling layers routed to the split-operand transposed kernel
(csrc/conv1d_split.hip, ``convtr1d_split_mfma_kernel``).  The admission tables are forced to "every
supported layer" (``_ConvNd.split_admit_all``), so that the short test inputs reach the kernel."""
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

CONVTR_KERNEL = "convtr1d_split_mfma_kernel"
SPLIT_KERNELS = (CONVTR_KERNEL, "conv1d_split_mfma_kernel", "resunit_split_kernel")


@pytest.fixture
def admit_all(monkeypatch):
    monkeypatch.setattr(_ConvNd, "split_exact", True)
    monkeypatch.setattr(_ConvNd, "split_admit_all", True)


def _v1(device, seed=5):
    g = HiFiGANGenerator(**synth.HIFIGAN_V1)
    sd = synth_for(g, seed, 1.25)
    g.load_state_dict(sd)
    return g.to(device).eval(), sd


def _launches(prof, kernel):
    r = prof.results.get(kernel)
    return 0 if r is None else int(r["launches"])


@pytest.mark.parametrize("batch,frames", [(2, 24), (1, 40)])
def test_generator_matches_oracle_and_switch_off_is_the_fp32_path(batch, frames, admit_all, device):
    g, sd = _v1(device)
    c = synth.synth_input("c", (batch, 80, frames), seed=frames)
    with torch.no_grad():
        ref = torch_cpu.hifigan_generator(sd, c, **synth.HIFIGAN_V1)
        with ops.profile() as prof:
            y = g(c.to(device)).clone()
        assert _launches(prof, CONVTR_KERNEL) == 4, sorted(prof.results)
        _ConvNd.split_exact = False
        with ops.profile() as prof_off:
            y_off = g(c.to(device)).clone()
        assert CONVTR_KERNEL not in prof_off.results
        _ConvNd.split_admit_all = False  # the admission table itself admits no launch this short
        _ConvNd.split_exact = True
        with ops.profile() as prof_dflt:
            y_dflt = g(c.to(device)).clone()
        assert CONVTR_KERNEL not in prof_dflt.results
    print(f"max abs vs oracle: split {max_abs(y, ref):.3e}, fp32 kernels {max_abs(y_off, ref):.3e}")
    assert y.shape == ref.shape
    assert max_abs(y, ref) <= WAVE_TOL
    assert max_abs(y_off, ref) <= WAVE_TOL
    assert torch.equal(y_off, y_dflt), "the switch turned off must leave exactly the default path"


def test_eager_graph_chained_forked_and_serial_are_bit_identical(admit_all, device):
    g, _ = _v1(device)
    c = synth.synth_input("c", (2, 80, 24), seed=24).to(device)
    with torch.no_grad():
        with ops.profile() as prof:
            serial = g(c).clone()
        assert _launches(prof, CONVTR_KERNEL) == 4
        assert torch.equal(GraphedInference(g)(c), serial), "replay differs from eager"
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


def test_a_forward_that_needs_gradients_launches_no_split_kernel(admit_all, device):
    g, _ = _v1(device)
    c = synth.synth_input("c", (1, 80, 24), seed=3).to(device)
    with ops.profile() as prof:
        y = g(c)  # parameters require grad
    assert y.requires_grad and not any(k in prof.results for k in SPLIT_KERNELS), sorted(prof.results)
    for p in g.parameters():
        p.requires_grad_(False)
    with ops.profile() as prof:
        y = g(c.clone().requires_grad_())  # only the input does
    assert y.requires_grad and not any(k in prof.results for k in SPLIT_KERNELS), sorted(prof.results)
    with ops.profile() as prof:
        g(c)  # nothing does: the inference path, grad mode on or off
    assert _launches(prof, CONVTR_KERNEL) == 4
