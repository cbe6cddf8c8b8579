"""GPU: the Parallel WaveGAN generator in bf16-operand inference mode (utils.set_inference_precision,
ParallelWaveGANGenerator.inference(precision=)); the residual layers run on the fused bf16 layer (csrc/wavenet_bf16.hip).

Whole generator, statistical, as tests/test_hifigan_bf16_gpu.py: bf16 rounding decisions flip on one-ulp differences and
the flips propagate through the layers, so no implementation matches the CPU emulation sample by sample.  The test
compares error against error, ``ratio = rms(y_gpu_bf16 - y_oracle_fp32) / rms(y_emulation - y_oracle_fp32)``, and
requires 0.5 <= ratio <= 2.  The upper bar is the project's HiFi-GAN bar; the lower bar catches a mode that is not
really on (the fp32 path gives a ratio near 1e-4).  The emulation's predicate mirrors which convolutions the GPU runs
in bf16.  No sample is left out of the RMS.  The ratio cannot tell a wrong rounding definition from a right one: the
stage test (tests/test_wavenet_bf16_gpu.py) does that.
"""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import torch_cpu
from parallelwavegan_amd import ops
from parallelwavegan_amd.graphs import GraphedInference
from parallelwavegan_amd.models import ParallelWaveGANGenerator
from parallelwavegan_amd.utils import get_inference_precision, set_inference_precision
from tests.bf16_emulation import bf16_operands, rms
from tests.golden import synth
from tests.util import WAVE_TOL, load_golden, max_abs, synth_for

LOWER, UPPER = 0.5, 2.0
N_V1 = 1 + 1 + 30 * 4 + 2  # conv_in, first_conv, four per residual layer, the two last 1x1 convolutions
N_CAUSAL, N_MELGAN_UP = 28, 47
# (frames, batch) x weight seeds
GENERATOR_CASES = [(f, b, s) for s in (5, 9) for f, b in ((1, 1), (7, 2), (40, 2), (100, 1))]
LAYER_KERNEL, FP32_LAYER_KERNEL, CONV_KERNEL = "wavenet_bf16_layer_kernel", "wavenet_layer_kernel", "conv1d_bf16_mfma_kernel"


def _v1(device, seed=5):
    g = ParallelWaveGANGenerator()
    sd = synth_for(g, seed, synth.PWG_G_SCALE)
    g.load_state_dict(sd)
    return g.to(device).eval(), sd


def _zc(frames, batch, seed, up=256, context=4):
    return (synth.synth_input("z", (batch, 1, frames * up), seed=seed),
            synth.synth_input("c", (batch, 80, frames + context), seed=seed))


def _ratio(y, ref, emu):
    e_gpu, e_emu = rms(y - ref), rms(emu - ref)
    return {"rms_gpu_bf16_minus_oracle": e_gpu, "rms_emulation_minus_oracle": e_emu, "ratio": e_gpu / e_emu,
            "rms_signal": rms(ref)}


def measure_case(frames, batch, seed, device):
    g, sd = _v1(device, seed)
    z, c = _zc(frames, batch, frames)
    with torch.no_grad():
        ref = torch_cpu.pwg_generator(sd, z, c)
        with bf16_operands() as st:
            emu = torch_cpu.pwg_generator(sd, z, c)
    assert st == {"rounded": N_V1, "untouched": 0}
    assert set_inference_precision(g, "bf16") == N_V1
    with torch.no_grad():
        y = g(z.to(device), c.to(device)).cpu()
    assert y.shape == ref.shape and torch.isfinite(y).all()
    return dict(frames=frames, batch=batch, seed=seed, **_ratio(y, ref, emu))


@pytest.mark.gpu
@pytest.mark.parametrize("frames,batch,seed", GENERATOR_CASES)
def test_bf16_generator_error_is_the_emulations_error(frames, batch, seed, device):
    m = measure_case(frames, batch, seed, device)
    print(m)
    assert m["rms_emulation_minus_oracle"] > 0
    assert LOWER <= m["ratio"] <= UPPER, m


def measure_causal(device):
    """Causal layers: the per-convolution path (no fused kernel), every convolution on the bf16 kernel."""
    cfg = synth.PWG_CAUSAL
    g = ParallelWaveGANGenerator(**copy.deepcopy(cfg))
    sd = synth_for(g, 7, synth.PWG_G_SCALE)
    g.load_state_dict(sd)
    g = g.to(device).eval()
    z, c = _zc(18, 2, 18, up=16, context=4)
    with torch.no_grad():
        ref = torch_cpu.pwg_generator_causal(sd, z, c, **cfg)
        with bf16_operands() as st:
            emu = torch_cpu.pwg_generator_causal(sd, z, c, **cfg)
        assert st == {"rounded": N_CAUSAL, "untouched": 0}
        assert set_inference_precision(g, "bf16") == N_CAUSAL
        g(z.to(device), c.to(device))
        with ops.profile() as prof:
            y = g(z.to(device), c.to(device)).cpu()
    assert prof.results[CONV_KERNEL]["launches"] == N_CAUSAL, prof.results
    assert LAYER_KERNEL not in prof.results and FP32_LAYER_KERNEL not in prof.results, prof.results
    assert not [k for k in prof.results if k.startswith("conv1d_") and k != CONV_KERNEL], prof.results
    return _ratio(y, ref, emu)


@pytest.mark.gpu
def test_causal_generator_takes_the_mode_per_convolution(device):
    m = measure_causal(device)
    print("causal", m)
    assert LOWER <= m["ratio"] <= UPPER, m


# ---- PWG with a MelGAN upsampler: oracle/ has no single function for it, so the test composes one
def melgan_upsampler_oracle(sd, c, cfg):
    """``melgan_generator`` (no final tanh) on the ``upsample_net.`` sub-state-dict."""
    up = cfg["upsample_params"]
    sub = {k[len("upsample_net."):]: v for k, v in sd.items() if k.startswith("upsample_net.")}
    return torch_cpu.melgan_generator(sub, c, kernel_size=up["kernel_size"], upsample_scales=up["upsample_scales"],
                                      stack_kernel_size=up["stack_kernel_size"], stacks=up["stacks"],
                                      use_final_nonlinear_activation=False)


def pwg_residual_oracle(sd, z, c, cfg):
    """The residual loop and output layers of ``torch_cpu.pwg_generator`` (copied: it starts from upsampled
    features ``c``)."""
    assert c.size(-1) == z.size(-1)
    get_weight, get_bias = torch_cpu.get_weight, torch_cpu.get_bias
    layers, stacks, kernel_size = cfg["layers"], cfg["stacks"], 3
    x = F.conv1d(z, get_weight(sd, "first_conv"), get_bias(sd, "first_conv"))
    skips = 0
    per_stack = layers // stacks
    for l in range(layers):
        p = f"conv_layers.{l}"
        d = 2 ** (l % per_stack)
        residual = x
        h = F.conv1d(x, get_weight(sd, p + ".conv"), get_bias(sd, p + ".conv"), dilation=d,
                     padding=(kernel_size - 1) // 2 * d)
        xa, xb = h.split(h.size(1) // 2, dim=1)
        a = F.conv1d(c, get_weight(sd, p + ".conv1x1_aux"))
        ca, cb = a.split(a.size(1) // 2, dim=1)
        g = torch.tanh(xa + ca) * torch.sigmoid(xb + cb)
        s = F.conv1d(g, get_weight(sd, p + ".conv1x1_skip"), get_bias(sd, p + ".conv1x1_skip"))
        x = (F.conv1d(g, get_weight(sd, p + ".conv1x1_out"), get_bias(sd, p + ".conv1x1_out")) + residual) * math.sqrt(0.5)
        skips = skips + s
    skips = skips * math.sqrt(1.0 / layers)
    x = F.conv1d(F.relu(skips), get_weight(sd, "last_conv_layers.1"), get_bias(sd, "last_conv_layers.1"))
    return F.conv1d(F.relu(x), get_weight(sd, "last_conv_layers.3"), get_bias(sd, "last_conv_layers.3"))


def _melgan_up_predicate(kind, x, w, kwargs):
    """What the GPU runs in bf16 in the MelGAN upsampler: its transposed and 1x1 convolutions; the reflect-padded ones
    (the k = 7 input / output convolutions and the dilated stack convolutions) stay fp32."""
    return kind == "conv_transpose1d" or w.shape[-1] == 1


def _melgan_up_model(seed):
    g = ParallelWaveGANGenerator(**copy.deepcopy(synth.PWG_MELGAN_UPSAMPLER))
    sd = synth.synth_state_dict(g.state_dict(), seed=seed, g_scale=synth.PWG_G_SCALE)
    g.load_state_dict(sd)
    return g, sd


def test_composed_melgan_upsampler_oracle_reproduces_the_golden():
    """CPU: the composition above is the reference's forward (the committed golden, fp32, within WAVE_TOL)."""
    gold = load_golden("pwg_melgan_upsampler")
    seed = int(gold["meta"][0])
    _, sd = _melgan_up_model(seed)
    c = synth.synth_input("c", (2, 80, 9), seed=seed)
    z = synth.synth_input("z", (2, 1, 9 * 256), seed=seed)
    cfg = synth.PWG_MELGAN_UPSAMPLER
    with torch.no_grad():
        y = pwg_residual_oracle(sd, z, melgan_upsampler_oracle(sd, c, cfg), cfg)
    assert max_abs(y, gold["y"]) <= WAVE_TOL


def measure_melgan_upsampler(device):
    cfg = synth.PWG_MELGAN_UPSAMPLER
    g, sd = _melgan_up_model(21)
    g = g.to(device).eval()
    z, c = _zc(12, 2, 12, context=0)
    with torch.no_grad():
        ref = pwg_residual_oracle(sd, z, melgan_upsampler_oracle(sd, c, cfg), cfg)
        # upsampler: its reflect-padded convolutions stay fp32; residual layers and the rest: all rounded
        with bf16_operands(_melgan_up_predicate) as st_up:
            c_emu = melgan_upsampler_oracle(sd, c, cfg)
        with bf16_operands() as st:
            emu = pwg_residual_oracle(sd, z, c_emu, cfg)
        assert set_inference_precision(g, "bf16") == N_MELGAN_UP
        assert st_up == {"rounded": 20, "untouched": 10} and st == {"rounded": 27, "untouched": 0}, (st_up, st)
        assert st_up["rounded"] + st["rounded"] == N_MELGAN_UP
        g(z.to(device), c.to(device))
        with ops.profile() as prof:
            y = g(z.to(device), c.to(device)).cpu()
    assert prof.results[LAYER_KERNEL]["launches"] == cfg["layers"] and FP32_LAYER_KERNEL not in prof.results
    return _ratio(y, ref, emu)


@pytest.mark.gpu
def test_melgan_upsampler_generator_takes_the_fused_layer(device):
    m = measure_melgan_upsampler(device)
    print("melgan upsampler", m)
    assert LOWER <= m["ratio"] <= UPPER, m


@pytest.mark.gpu
def test_mode_is_really_on_and_default_is_untouched(device):
    g, _ = _v1(device)
    untouched, _ = _v1(device)
    z, c = (t.to(device) for t in _zc(40, 2, 40))
    with torch.no_grad():
        y_never = untouched(z, c)
        y_fp32 = g(z, c)
        assert torch.equal(y_fp32, y_never)
        assert set_inference_precision(g, "bf16") == N_V1 and get_inference_precision(g) == "bf16"
        with ops.profile() as prof_up:
            g.upsample_net(c)
        upsampler = set(prof_up.results)
        assert "stretch_conv_fwd_kernel" in upsampler and CONV_KERNEL in upsampler, upsampler  # conv_in: bf16
        g(z, c)  # (weight images built outside the profiled forward)
        with ops.profile() as prof:
            y_bf16 = g(z, c)
        assert not torch.equal(y_bf16, y_fp32)
        assert prof.results[LAYER_KERNEL]["launches"] == 30, prof.results
        assert FP32_LAYER_KERNEL not in prof.results, prof.results
        assert not [k for k in prof.results if k.startswith("conv1d_") and k != CONV_KERNEL], prof.results
        # conv_in, first_conv and the two last 1x1 convolutions on the bf16 convolution kernel
        assert prof.results[CONV_KERNEL]["launches"] == 4, prof.results
        assert set(prof.results) == upsampler | {LAYER_KERNEL, CONV_KERNEL}, prof.results
        assert torch.equal(g(z, c), y_bf16)  # deterministic
        # back to fp32: bit-identical to a model that never saw the switch, on the fp32 kernels
        assert set_inference_precision(g, "fp32") == N_V1
        with ops.profile() as prof:
            y_back = g(z, c)
        assert torch.equal(y_back, y_never)
        assert LAYER_KERNEL not in prof.results and prof.results[FP32_LAYER_KERNEL]["launches"] == 30


@pytest.mark.gpu
def test_inference_keyword_gradients_and_weight_updates(device):
    g, _ = _v1(device)
    f = synth.synth_input("c", (1, 80, 30), seed=30)[0].transpose(0, 1).contiguous().to(device)
    noise = synth.synth_input("z", (30 * 256, 1), seed=30).to(device)  # (the context frames are added by inference)
    y32 = g.inference(f, noise)
    assert torch.is_grad_enabled() and next(g.parameters()).requires_grad
    y16 = g.inference(f, noise, precision="bf16")
    assert y16.shape == y32.shape and not torch.equal(y16, y32.detach()) and not y16.requires_grad
    assert all(m.precision == "fp32" for m in g.modules() if hasattr(m, "precision"))  # the keyword is per call
    assert torch.equal(g.inference(f, noise).detach(), y32.detach())
    set_inference_precision(g, "bf16")
    assert torch.equal(g.inference(f, noise), y16)  # None = what was set on the model
    assert torch.equal(g.inference(f, noise, precision="fp32").detach(), y32.detach())
    assert get_inference_precision(g) == "bf16"
    # a gradient-requiring call raises before any launch, also where the fused bf16 layer is eligible
    z, c = (t.to(device) for t in _zc(8, 1, 8))
    with pytest.raises(RuntimeError, match="bf16 inference precision"):
        g(z, c)
    blk = g.conv_layers[9]  # dilation 512: the stand-alone bf16 kernel cannot take its dilated convolution
    x = torch.randn(1, 64, 2048, device=device)
    ca = torch.randn(1, 80, 2048, device=device)
    with torch.no_grad():
        blk(x, ca)
        with ops.profile() as prof:
            blk(x, ca)
    assert set(prof.results) == {LAYER_KERNEL}
    with pytest.raises(RuntimeError, match="bf16 inference precision"), ops.profile() as prof:
        blk(x, ca)
    with torch.no_grad(), pytest.raises(RuntimeError, match="bf16 inference precision"), ops.profile() as prof2:
        with torch.enable_grad():
            for p in blk.parameters():
                p.requires_grad_(False)
            blk(x.requires_grad_(), ca)
    for p in blk.parameters():
        p.requires_grad_(True)
    assert not prof.results and not prof2.results  # nothing was launched
    # a block that cannot take the fused launch and whose convolution cannot run in bf16 alone names the reason
    with torch.no_grad(), pytest.raises(RuntimeError, match="no aux input"):
        blk(x.detach(), None)
    # the bf16 layer image follows the parameters like the fp32 one: load_state_dict, remove_weight_norm
    other = synth_for(g, 6, synth.PWG_G_SCALE)
    g.load_state_dict(other)
    y_other = g.inference(f, noise)
    assert not torch.equal(y_other, y16)
    fresh = ParallelWaveGANGenerator()
    fresh.load_state_dict(other)
    fresh = fresh.to(device).eval()
    set_inference_precision(fresh, "bf16")
    assert torch.equal(fresh.inference(f, noise), y_other)
    g.remove_weight_norm()
    y_baked = g.inference(f, noise)  # (the baked weight may differ from g * v / |v| by an ulp: statistical comparison)
    assert rms(y_baked - y_other) <= UPPER * rms(y_other - g.inference(f, noise, precision="fp32").detach())


@pytest.mark.gpu
def test_graph_replay_equals_eager_and_follows_the_precision(device):
    g, _ = _v1(device)
    z, c = (t.to(device) for t in _zc(50, 2, 50))
    with torch.no_grad():
        e32 = g(z, c).clone()
        run = GraphedInference(g)
        assert torch.equal(run(z, c), e32)
        set_inference_precision(g, "bf16")
        e16 = g(z, c).clone()
        r16 = run(z, c).clone()  # the precision is part of the compared state: the fp32 graph is dropped
        assert torch.equal(r16, e16) and not torch.equal(r16, e32)
        assert torch.equal(run(z, c), r16)  # replay is deterministic
        set_inference_precision(g, "fp32")
        assert torch.equal(run(z, c), e32)
        set_inference_precision(g, "bf16")
        assert torch.equal(run(z, c), e16)
