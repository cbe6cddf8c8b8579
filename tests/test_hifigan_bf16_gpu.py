"""GPU: the HiFi-GAN generator in bf16-operand inference mode (utils.set_inference_precision / inference(precision=)).

Whole generator, statistical: bf16 rounding decisions flip on one-ulp differences and the flips propagate through ~50
layers, so no implementation matches the CPU emulation sample by sample (the emulation accumulated in fp32 and in
float64 differ from each other by as much as either differs from the fp32 oracle).  The test compares error against
error: ``rms(y_gpu_bf16 - y_oracle_fp32) <= 2 * rms(y_emulation - y_oracle_fp32)``; both sides are realisations of the
same rounding process, a real defect (dropped tap, wrong polyphase row, stale LDS element) puts the error RMS near the
signal RMS, more than 100 x over.  No sample is left out of the RMS.
"""
import pytest
import torch

from oracle import torch_cpu
from parallelwavegan_amd import ops
from parallelwavegan_amd.graphs import GraphedInference
from parallelwavegan_amd.models import HiFiGANGenerator
from parallelwavegan_amd.utils import set_inference_precision, streaming
from tests.bf16_emulation import bf16_operands, rms
from tests.golden import synth
from tests.util import synth_for

pytestmark = pytest.mark.gpu

FACTOR = 2.0
# (frames, batch, weight seed): the cases of test_hifigan_gpu.py::test_generator_matches_oracle_various_lengths + 2 x 800
GENERATOR_CASES = [(1, 1, 5), (7, 2, 5), (100, 1, 5), (33, 3, 5), (800, 2, 9)]
BF16_KERNEL, FP32_KERNEL = "conv1d_bf16_mfma_kernel", "conv1d_mfma_dma_kernel"
N_CONVS_V1 = 1 + 4 + 12 * 6 + 1


def _v1(device, seed=5):
    g = HiFiGANGenerator(**synth.HIFIGAN_V1)
    sd = synth_for(g, seed, 1.25)
    g.load_state_dict(sd)
    return g.to(device).eval(), sd


def _oracle_and_emulation(sd, c):
    with torch.no_grad():
        ref = torch_cpu.hifigan_generator(sd, c, **synth.HIFIGAN_V1)
        with bf16_operands():
            emu = torch_cpu.hifigan_generator(sd, c, **synth.HIFIGAN_V1)
    return ref, emu


def measure_case(frames, batch, seed, device):
    g, sd = _v1(device, seed)
    c = synth.synth_input("c", (batch, 80, frames), seed=frames)
    ref, emu = _oracle_and_emulation(sd, c)
    assert set_inference_precision(g, "bf16") == N_CONVS_V1
    with torch.no_grad():
        y = g(c.to(device)).cpu()
    assert y.shape == ref.shape and torch.isfinite(y).all()
    e_gpu, e_emu = rms(y - ref), rms(emu - ref)
    return {"frames": frames, "batch": batch, "rms_gpu_bf16_minus_oracle": e_gpu, "rms_emulation_minus_oracle": e_emu,
            "ratio": e_gpu / e_emu, "rms_signal": rms(ref), "max_abs_gpu_bf16_minus_oracle": float((y - ref).abs().max())}


@pytest.mark.parametrize("frames,batch,seed", GENERATOR_CASES)
def test_bf16_generator_error_is_the_emulations_error(frames, batch, seed, device):
    m = measure_case(frames, batch, seed, device)
    print(m)
    assert m["rms_emulation_minus_oracle"] > 0
    assert m["rms_gpu_bf16_minus_oracle"] <= FACTOR * m["rms_emulation_minus_oracle"], m


def test_causal_generator_takes_the_mode(device):
    """Left-only padding and the trimmed causal transposed convolution (padding = stride) run on the same kernel."""
    cfg = synth.HIFIGAN_CAUSAL
    g = HiFiGANGenerator(**cfg)
    sd = synth_for(g, 7, 1.25)
    g.load_state_dict(sd)
    g = g.to(device).eval()
    c = synth.synth_input("c", (2, 80, 37), seed=37)
    with torch.no_grad():
        ref = torch_cpu.hifigan_generator_causal(sd, c, **cfg)
        with bf16_operands():
            emu = torch_cpu.hifigan_generator_causal(sd, c, **cfg)
        n = set_inference_precision(g, "bf16")
        with ops.profile() as prof:
            y = g(c.to(device)).cpu()
    assert n == prof.results[BF16_KERNEL]["launches"] and FP32_KERNEL not in prof.results
    e_gpu, e_emu = rms(y - ref), rms(emu - ref)
    print(f"causal: rms {e_gpu:.3e} vs emulation {e_emu:.3e} (ratio {e_gpu / e_emu:.3f})")
    assert 0 < e_gpu <= FACTOR * e_emu


def test_mode_is_really_on_and_default_is_untouched(device):
    g, sd = _v1(device)
    untouched, _ = _v1(device)
    c = synth.synth_input("c", (2, 80, 40), seed=40).to(device)
    with torch.no_grad():
        y_never = untouched(c)
        y_fp32 = g(c)
        assert torch.equal(y_fp32, y_never)
        assert set_inference_precision(g, "bf16") == N_CONVS_V1
        g(c)  # (weight images built outside the profiled forward)
        with ops.profile() as prof:
            y_bf16 = g(c)
        assert not torch.equal(y_bf16, y_fp32)
        assert prof.results[BF16_KERNEL]["launches"] == N_CONVS_V1, prof.results
        assert FP32_KERNEL not in prof.results and "resunit_kernel" not in " ".join(prof.results), prof.results
        assert set(prof.results) == {BF16_KERNEL}, prof.results  # no other kernel of the library ran
        y_again = g(c)
        assert torch.equal(y_again, y_bf16)  # deterministic
        # back to fp32: bit-identical to a model that never saw the switch, on the fp32 kernels
        assert set_inference_precision(g, "fp32") == N_CONVS_V1
        with ops.profile() as prof:
            y_back = g(c)
        assert torch.equal(y_back, y_never)
        assert BF16_KERNEL not in prof.results


def test_inference_keyword_and_weight_updates(device):
    g, sd = _v1(device)
    f = synth.synth_input("c", (1, 80, 30), seed=30)[0].transpose(0, 1).contiguous().to(device)
    y32 = g.inference(f)
    # grad mode is on and the parameters require grad: the keyword runs the forward under no_grad itself
    assert torch.is_grad_enabled() and next(g.parameters()).requires_grad
    y16 = g.inference(f, precision="bf16")
    assert y16.shape == y32.shape and not torch.equal(y16, y32) and not y16.requires_grad
    assert all(m.precision == "fp32" for m in g.modules() if hasattr(m, "precision"))  # the keyword is per call
    assert torch.equal(g.inference(f).detach(), y32.detach())
    set_inference_precision(g, "bf16")
    assert torch.equal(g.inference(f), y16)  # None = what was set on the model
    assert torch.equal(g.inference(f, precision="fp32").detach(), y32.detach())
    # a gradient-requiring call raises
    with pytest.raises(RuntimeError, match="bf16 inference precision"):
        g(f.transpose(0, 1).unsqueeze(0).contiguous())
    with torch.no_grad(), pytest.raises(RuntimeError, match="bf16 inference precision"):
        with torch.enable_grad():
            g(f.transpose(0, 1).unsqueeze(0).contiguous().requires_grad_())
    # the bf16 weight image follows the parameters like the fp32 one: load_state_dict, remove_weight_norm
    other = synth_for(g, 6, 1.25)
    g.load_state_dict(other)
    y_other = g.inference(f)
    assert not torch.equal(y_other, y16)
    fresh = HiFiGANGenerator(**synth.HIFIGAN_V1)
    fresh.load_state_dict(other)
    fresh = fresh.to(device).eval()
    set_inference_precision(fresh, "bf16")
    assert torch.equal(fresh.inference(f), y_other)
    g.remove_weight_norm()
    y_baked = g.inference(f)  # (the baked fp32 weight may differ from g * v / |v| by an ulp: statistical comparison)
    assert rms(y_baked - y_other) <= FACTOR * rms(y_other.detach() - g.inference(f, precision="fp32").detach())


def test_graph_replay_equals_eager_and_follows_the_precision(device):
    g, sd = _v1(device)
    c = synth.synth_input("c", (2, 80, 50), seed=50).to(device)
    with torch.no_grad():
        e32 = g(c).clone()
        run = GraphedInference(g)
        assert torch.equal(run(c), e32)
        set_inference_precision(g, "bf16")
        e16 = g(c).clone()
        r16 = run(c).clone()  # the precision is part of the compared state: the fp32 graph is dropped
        assert torch.equal(r16, e16) and not torch.equal(r16, e32)
        assert torch.equal(run(c), r16)  # replay is deterministic
        set_inference_precision(g, "fp32")
        assert torch.equal(run(c), e32)
        set_inference_precision(g, "bf16")
        assert torch.equal(run(c), e16)


def test_branch_streams_chained_forked_and_serial_are_bit_identical_in_bf16(device):
    """Mirror of test_hifigan_gpu.py::test_chained_branch_ends_equal_the_serial_running_sum; the chained epilogue add
    arrives through add1 / add2 of the bf16 kernel.  Eager and captured (branches fork only inside a capture)."""
    torch.manual_seed(3)
    g = HiFiGANGenerator(channels=128, upsample_scales=(4, 4), upsample_kernel_sizes=(8, 8)).to(device).eval()
    assert set_inference_precision(g, "bf16") > 0
    c = torch.randn(2, 80, 64, device=device)
    with torch.no_grad():
        serial = g(c).clone()
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


def test_chunked_synthesizer_on_a_bf16_model(device):
    """ChunkedSynthesizer works unchanged on a model in bf16 mode; its output meets the whole-generator bar against
    the fp32 oracle (the fp32 streaming bar against the full forward does not carry over: a chunk-edge difference of
    one ulp flips later bf16 roundings)."""
    g, sd = _v1(device, 11)
    gen = torch.Generator().manual_seed(3)
    feats = [torch.randn(n, 80, generator=gen) for n in (300, 77)]
    set_inference_precision(g, "bf16")
    syn = streaming.ChunkedSynthesizer(g, chunk_frames=64, max_batch=4)
    outs = syn.synthesize_many(feats)
    for f, y in zip(feats, outs):
        c = f.transpose(0, 1).unsqueeze(0).contiguous()
        ref, emu = _oracle_and_emulation(sd, c)
        y = y.cpu().reshape(ref.shape)
        assert torch.isfinite(y).all()
        e_gpu, e_emu = rms(y - ref), rms(emu - ref)
        print(f"chunked {f.shape[0]} frames: rms {e_gpu:.3e} vs emulation {e_emu:.3e} (ratio {e_gpu / e_emu:.3f})")
        assert e_gpu <= FACTOR * e_emu
