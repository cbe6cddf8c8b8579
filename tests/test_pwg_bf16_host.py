"""CPU: host side of the bf16-operand inference mode of the Parallel WaveGAN generator (csrc/wavenet_bf16.hip: the
fused bf16 residual layer).  No GPU needed."""
import copy
import ctypes
import inspect

import pytest
import torch

from parallelwavegan_amd import _lib, ops
from parallelwavegan_amd.layers.conv import _ConvNd
from parallelwavegan_amd.models import ParallelWaveGANGenerator
from parallelwavegan_amd.utils import get_inference_precision, set_inference_precision
from tests.golden import synth


def _convs(model):
    return [m for m in model.modules() if isinstance(m, _ConvNd)]


def test_new_symbols_are_exported():
    for name in ("pwg_wavenet_bf16_supported", "pwg_wavenet_bf16_packed_weight_bytes", "pwg_wavenet_bf16_pack_weights",
                 "pwg_wavenet_bf16_layer_forward", "pwg_wavenet_bf16_layer_forward_cfg"):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name)


@pytest.mark.parametrize("batch,t,dil", [(1, 1, 1), (1, 1, 512), (16, 102400, 512), (2, 7, 2), (65535, 64, 4),
                                         (3, 777, 64), (1, 50, 256)])
def test_supported_covers_the_pwg_v1_geometry(batch, t, dil):
    d = ops.make_wavenet_desc(batch, t, dil, out_mul=0.5 ** 0.5)
    assert ops.wavenet_bf16_supported(d), _lib.lib().pwg_last_error()
    assert ops.wavenet_layer_supported(d)  # the same geometry as the fp32 one-launch layer


@pytest.mark.parametrize("kwargs,reason", [
    (dict(causal=True), b"causal"),
    (dict(aux_channels=64), b"aux_channels"),
    (dict(residual_channels=32), b"residual"),
    (dict(gate_channels=256), b"gate"),
    (dict(kernel=5), b"kernel"),
])
def test_unsupported_geometries_name_the_reason(kwargs, reason):
    d = ops.make_wavenet_desc(2, 100, 4, **kwargs)
    assert not ops.wavenet_bf16_supported(d)
    assert reason in _lib.lib().pwg_last_error()
    assert _lib.lib().pwg_wavenet_bf16_packed_weight_bytes(ctypes.byref(d)) == 0


def test_unsupported_sizes_name_the_reason():
    assert not ops.wavenet_bf16_supported(ops.make_wavenet_desc(65536, 64, 1))
    assert b"batch" in _lib.lib().pwg_last_error()
    assert not ops.wavenet_bf16_supported(ops.make_wavenet_desc(1, 0, 1))
    assert b"t = 0" in _lib.lib().pwg_last_error()


def test_packed_weight_bytes():
    # phase 1: K = 3 * 64 + 80 padded to 288, phase 2: K = 64; 128 rows each; bf16
    d = ops.make_wavenet_desc(1, 64, 1)
    assert ops.wavenet_bf16_packed_weight_bytes(d) == (288 + 64) * 128 * 2


def test_inference_accepts_precision():
    assert "precision" in inspect.signature(ParallelWaveGANGenerator.inference).parameters
    with pytest.raises(ValueError):
        ParallelWaveGANGenerator(**copy.deepcopy(synth.PWG_CAUSAL)).inference(torch.zeros(4, 80), precision="fp16")


@pytest.mark.parametrize("cfg,n_bf16,n_all", [
    (None, 124, 124),                                                  # PWG.v1: every convolution, dilation 512 included
    ("PWG_CAUSAL", 28, 28),                                            # per-convolution path
    ("PWG_MELGAN_UPSAMPLER", 47, 57),                                  # 10 reflect-padded upsampler convolutions: fp32
])
def test_set_inference_precision_counts(cfg, n_bf16, n_all):
    g = ParallelWaveGANGenerator(**copy.deepcopy(getattr(synth, cfg))) if cfg else ParallelWaveGANGenerator()
    convs = _convs(g)
    assert len(convs) == n_all
    assert set_inference_precision(g, "bf16") == n_bf16
    assert sum(m.precision == "bf16" for m in convs) == n_bf16 and get_inference_precision(g) == "bf16"
    assert set_inference_precision(g, "fp32") == n_all
    assert all(m.precision == "fp32" for m in convs)


def test_dilation_512_blocks_are_covered_by_the_fused_layer():
    g = ParallelWaveGANGenerator()
    set_inference_precision(g, "bf16")
    for i in (9, 19, 29):
        blk = g.conv_layers[i]
        assert blk.conv.dilation == 512 and not blk.conv.bf16_capable()  # the stand-alone kernel cannot take it ...
        assert blk.conv.precision == "bf16" and blk.bf16_covered_convs() == blk.fused_convs()  # ... the layer can


def test_reflect_padded_upsampler_convolutions_stay_fp32():
    g = ParallelWaveGANGenerator(**copy.deepcopy(synth.PWG_MELGAN_UPSAMPLER))
    set_inference_precision(g, "bf16")
    up = _convs(g.upsample_net)
    assert sum(m.pad_mode == "reflect" for m in up) == 10
    for m in up:
        assert (m.precision == "bf16") == (m.pad_mode == "zero")


def test_gradient_requiring_call_raises_before_any_launch():
    """The check sits in front of the fused path and of any device work: on CPU tensors it raises on the host."""
    g = ParallelWaveGANGenerator(**copy.deepcopy(synth.PWG_CAUSAL))
    set_inference_precision(g, "bf16")
    blk = g.conv_layers[0]
    with pytest.raises(RuntimeError, match="bf16 inference precision"):
        blk(torch.zeros(1, 64, 8), torch.zeros(1, 80, 8))
    v1 = ParallelWaveGANGenerator()
    set_inference_precision(v1, "bf16")
    with pytest.raises(RuntimeError, match="bf16 inference precision"):
        v1.conv_layers[9](torch.zeros(1, 64, 8), torch.zeros(1, 80, 8))
