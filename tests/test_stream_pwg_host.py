"""CPU: host logic of the causal Parallel WaveGAN stream (csrc/wavenet_stream.hip, pwg_stretch_conv_stream,
utils.PWGStream) -- entry points, geometry answers, history shapes and refusals.  No launch."""
import ctypes
import os
import re

import pytest
import torch

from parallelwavegan_amd import _lib, layers, models, ops, utils
from tests.golden import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _err():
    return _lib.lib().pwg_last_error().decode(errors="replace")


def test_entry_points_are_additive():
    """Four new symbols, declared, exported and bound; no existing signature changed, so the ABI version stays 15."""
    assert _lib.ABI_VERSION == 15 == _lib.lib().pwg_abi_version()
    header = open(os.path.join(ROOT, "include", "pwg_kernels.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for ret, name in (("int", "pwg_wavenet_stream_supported"), ("size_t", "pwg_wavenet_stream_hist_floats"),
                      ("int", "pwg_wavenet_stream_forward"), ("int", "pwg_stretch_conv_stream")):
        assert re.search(r"\b" + ret + " " + name + r"\(", header), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    for name in ("wavenet_stream_supported", "wavenet_stream_hist_floats", "wavenet_stream_forward", "stretch_conv_stream"):
        assert callable(getattr(ops, name)), name
    assert "pwg_abi_version() stays 15" in header


def test_layer_geometry_answers_without_a_gpu():
    for d in range(1, 513):
        for batch in (1, 16):
            for n in (1, 63, 64, 1024):
                desc = ops.make_wavenet_desc(batch, n, d, causal=True)
                assert ops.wavenet_stream_supported(desc), (d, batch, n, _err())
                assert ops.wavenet_stream_hist_floats(desc) == batch * 64 * 2 * d
    assert ops.wavenet_stream_supported(ops.make_wavenet_desc(2, 7, 3, causal=True))  # any dilation >= 1
    bad = [(dict(causal=False), "causal"), (dict(causal=True, kernel=5), "kernel"),
           (dict(causal=True, residual_channels=32), "channels"), (dict(causal=True, aux_channels=64), "aux")]
    for kw, word in bad:
        desc = ops.make_wavenet_desc(1, 64, 2, **kw)
        assert not ops.wavenet_stream_supported(desc), kw
        assert word in _err(), (kw, _err())
        assert ops.wavenet_stream_hist_floats(desc) == 0
    desc = ops.make_wavenet_desc(0, 64, 2, causal=True)
    assert not ops.wavenet_stream_supported(desc) and "batch" in _err()
    assert ops.wavenet_stream_hist_floats(desc) == 0


def test_stream_layers_and_history_shapes():
    m = models.ParallelWaveGANGenerator(**synth.PWG_CAUSAL)
    sl = m.stream_layers()
    assert len(sl) == 1 + 2 + 6
    B = 3
    shapes = [tuple(layer.history_shape(B)) for layer, _ in sl]
    assert shapes == [(B, 80, 2)] + [(B, 80, 2)] * 2 + [(B, 64, 2 * d) for d in (1, 2, 4, 1, 2, 4)]
    assert [rate for _, rate in sl] == [1, 1, 4] + [16] * 6
    # every block's shape is what the kernel says it keeps
    for layer, _ in sl[3:]:
        assert ops.wavenet_stream_hist_floats(layer.stream_desc(B, 5)) == torch.Size(layer.history_shape(B)).numel()
    assert ops.conv1d_stream_hist_floats(sl[0][0].stream_desc(B, 5)) == B * 80 * 2
    v1 = models.ParallelWaveGANGenerator(use_causal_conv=True)
    blocks = [layer for layer, _ in v1.stream_layers() if isinstance(layer, layers.WaveNetResidualBlock)]
    assert len(blocks) == 30 and sum(layer.history_shape(1)[2] for layer in blocks) == 6138
    assert len(v1.stream_layers()) == 1 + 4 + 30
    # the upsample networks on their own
    assert len(m.upsample_net.stream_layers()) == 3 and len(m.upsample_net.upsample.stream_layers()) == 2
    with pytest.raises(ValueError, match="use_causal_conv"):
        models.ParallelWaveGANGenerator(**dict(synth.PWG_CAUSAL, use_causal_conv=False)).upsample_net.stream_layers()


def test_block_stream_forward_refusals():
    x, c = torch.zeros(1, 64, 8), torch.zeros(1, 80, 8)
    blk = layers.WaveNetResidualBlock(dilation=2, use_causal_conv=True)
    h = [torch.zeros(blk.history_shape(1)) for _ in range(2)]
    assert blk.history_shape(4) == (4, 64, 4)
    with pytest.raises(ValueError, match="use_causal_conv"):
        layers.WaveNetResidualBlock(dilation=2).stream_forward(x, c, None, h[0])
    small = layers.WaveNetResidualBlock(residual_channels=32, gate_channels=64, skip_channels=32, use_causal_conv=True)
    with pytest.raises(RuntimeError, match="channels"):
        small.stream_forward(torch.zeros(1, 32, 8), c, None, torch.zeros(small.history_shape(1)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        blk.stream_forward(x, c, None, h[0])
    blk.conv.precision = "bf16"
    with pytest.raises(RuntimeError, match="bf16"):
        blk.stream_forward(x, c, None, h[0])


def test_pwgstream_refusals_come_before_the_device_check():
    cfg = synth.PWG_CAUSAL
    with pytest.raises(ValueError, match="use_causal_conv"):
        utils.PWGStream(models.ParallelWaveGANGenerator(**dict(cfg, use_causal_conv=False)))
    mel_up = models.ParallelWaveGANGenerator(
        layers=6, stacks=2, use_causal_conv=True, aux_context_window=0, upsample_net="MelGANGenerator",
        upsample_params=dict(upsample_scales=[4, 4], in_channels=80, out_channels=80, channels=64, stacks=1))
    with pytest.raises(ValueError, match="MelGANGenerator"):
        utils.PWGStream(mel_up)
    with pytest.raises(ValueError, match="upsample_conditional_features"):
        utils.PWGStream(models.ParallelWaveGANGenerator(**dict(cfg, upsample_conditional_features=False)))
    linear = models.ParallelWaveGANGenerator(**cfg)
    linear.upsample_net.upsample.up_layers[0].mode = "linear"  # (the constructor builds only "nearest")
    with pytest.raises(ValueError, match="nearest"):
        utils.PWGStream(linear)
    with pytest.raises(ValueError, match="freq_axis_kernel_size"):
        utils.PWGStream(models.ParallelWaveGANGenerator(
            **dict(cfg, upsample_params={"upsample_scales": [4, 4], "freq_axis_kernel_size": 3})))
    with pytest.raises(ValueError, match=r"channels = 32 / 64 / 32"):  # the kernel's own reason (pwg_last_error)
        utils.PWGStream(models.ParallelWaveGANGenerator(**dict(cfg, residual_channels=32, gate_channels=64,
                                                               skip_channels=32)))
    bf16 = models.ParallelWaveGANGenerator(**cfg)
    utils.set_inference_precision(bf16, "bf16")
    with pytest.raises(ValueError, match="bf16"):
        utils.PWGStream(bf16)
    with pytest.raises(ValueError, match="HiFiGANGenerator"):
        utils.PWGStream(models.HiFiGANGenerator(**synth.HIFIGAN_CAUSAL))
    with pytest.raises(ValueError, match="batch"):
        utils.PWGStream(models.ParallelWaveGANGenerator(**cfg), batch=0)
    # a supported causal model on the CPU: only the device is missing
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        utils.PWGStream(models.ParallelWaveGANGenerator(**cfg))
    # and CausalStream still names the class it cannot take (before its device check)
    with pytest.raises(ValueError, match="ParallelWaveGANGenerator"):
        utils.CausalStream(models.ParallelWaveGANGenerator(**cfg))
    assert utils.PWGStream.warmup_frames == 1
