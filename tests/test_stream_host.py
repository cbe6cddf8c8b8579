"""CPU: host logic of the streaming convolution (pwg_conv1d_stream_*) and of utils.CausalStream -- what the kernel
covers, the size of a layer's history, which models a stream accepts, and the warm-up a reflect-padded start needs.
Nothing here launches a kernel."""
import ctypes

import pytest
import torch

from parallelwavegan_amd import _lib, layers, models, ops
from parallelwavegan_amd.utils import CausalStream
from tests.golden import synth

HIFIGAN_V1_CAUSAL = dict(synth.HIFIGAN_V1, use_causal_conv=True)


def _why():
    return _lib.lib().pwg_last_error().decode()


@pytest.mark.parametrize("cls,cfg", [(models.HiFiGANGenerator, synth.HIFIGAN_CAUSAL),
                                     (models.MelGANGenerator, synth.MELGAN_CAUSAL),
                                     (models.HiFiGANGenerator, HIFIGAN_V1_CAUSAL)])
def test_stream_kernel_accepts_the_causal_layers(cls, cfg):
    m = cls(**cfg)
    stream_layers = m.stream_layers()
    assert len(stream_layers) >= 8
    for batch, n in ((1, 1), (2, 8), (16, 40)):
        for layer, rate in stream_layers:
            d = layer.stream_desc(batch, n * rate)
            assert ops.conv1d_stream_supported(d), (layer, _why())
            if isinstance(layer, layers.CausalConvTranspose1d):
                cv, h = layer.deconv, 1
                assert d.transposed == 1 and d.kernel == 2 * d.stride and d.pad_left == d.stride
                assert d.t_out == d.t_in * d.stride
            else:
                cv, h = layer.conv, (layer.conv.kernel_size - 1) * layer.conv.dilation
                assert d.transposed == 0 and d.pad_left == h and d.t_out == d.t_in
            assert ops.conv1d_stream_hist_floats(d) == batch * cv.in_channels * h
            assert tuple(layer.history_shape(batch)) == (batch, cv.in_channels, h)


def test_hist_floats_formula():
    d = ops.make_conv_desc(3, 24, 40, 9, 9, 5, dilation=3, pad_left=12)
    assert ops.conv1d_stream_hist_floats(d) == 3 * 24 * (5 - 1) * 3
    dt = ops.make_conv_desc(3, 24, 12, 9, 36, 8, stride=4, pad_left=4, transposed=True)
    assert ops.conv1d_stream_hist_floats(dt) == 3 * 24
    d1 = ops.make_conv_desc(2, 8, 8, 5, 5, 1)  # a 1 x 1 layer is causal and keeps nothing
    assert ops.conv1d_stream_supported(d1) and ops.conv1d_stream_hist_floats(d1) == 0


@pytest.mark.parametrize("name,desc,word", [
    ("grouped", lambda: ops.make_conv_desc(1, 16, 16, 8, 8, 3, pad_left=2, groups=4), "groups"),
    ("strided", lambda: ops.make_conv_desc(1, 16, 16, 8, 4, 3, stride=2, pad_left=2), "stride"),
    ("(k,1) width", lambda: ops.make_conv_desc(1, 16, 16, 8, 8, 3, pad_left=2, width=3), "width"),
    ("two-sided padding", lambda: layers.Conv1d(16, 16, 7, padding=3).make_desc(1, 8), "causal"),
    ("k != 2s transposed", lambda: ops.make_conv_desc(1, 16, 8, 8, 24, 7, stride=3, pad_left=3, transposed=True),
     "kernel"),
    ("non-causal transposed padding", lambda: layers.ConvTranspose1d(16, 8, 8, 4, padding=2).make_desc(1, 8), "padding"),
    ("reflected transposed start", lambda: ops.make_conv_desc(1, 16, 8, 8, 32, 8, stride=4, pad_left=4, transposed=True,
                                                              pad_mode="reflect"), "reflect"),
    ("tanh pre-activation", lambda: ops.make_conv_desc(1, 16, 16, 8, 8, 3, pad_left=2, pre_act="tanh"), "pre_act"),
    ("history beyond the LDS window", lambda: ops.make_conv_desc(1, 16, 16, 8, 8, 3, dilation=100, pad_left=200), "LDS"),
])
def test_stream_kernel_rejects_with_a_reason(name, desc, word):
    d = desc()
    assert not ops.conv1d_stream_supported(d), name
    assert word in _why(), (name, _why())
    assert ops.conv1d_stream_hist_floats(d) == 0


def test_stream_forward_refuses_cpu_tensors():
    d = ops.make_conv_desc(1, 4, 4, 8, 8, 3, pad_left=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.conv1d_stream_forward(d, torch.zeros(1, 4, 8), None, torch.zeros(1, 4, 2), torch.zeros(3 * 16 * 128))
    conv = layers.CausalConv1d(4, 4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv.stream_forward(torch.zeros(1, 4, 8), None, torch.zeros(conv.history_shape(1)))


def test_causal_stream_on_a_cpu_model_has_no_fallback():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CausalStream(models.HiFiGANGenerator(**synth.HIFIGAN_CAUSAL))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CausalStream(models.MelGANGenerator(**synth.MELGAN_CAUSAL), batch=2, use_graph=False)


def test_causal_stream_refuses_models_it_cannot_stream():
    with pytest.raises(ValueError, match="use_causal_conv"):
        CausalStream(models.HiFiGANGenerator(**synth.HIFIGAN_TINY))
    with pytest.raises(ValueError, match="use_causal_conv"):
        CausalStream(models.MelGANGenerator(channels=64, upsample_scales=[4, 2, 2], stacks=2))
    with pytest.raises(ValueError, match="PQMF"):  # multi-band: 4 sub-bands out
        CausalStream(models.MelGANGenerator(out_channels=4, channels=64, upsample_scales=[2, 2], stacks=2,
                                            use_causal_conv=True))
    with pytest.raises(ValueError, match="PQMF"):
        CausalStream(models.HiFiGANGenerator(**dict(synth.HIFIGAN_CAUSAL, out_channels=4)))
    with pytest.raises(ValueError, match="ParallelWaveGANGenerator"):
        CausalStream(models.ParallelWaveGANGenerator(**synth.PWG_CAUSAL))
    # a causal layer the kernel turns down: the reason comes from pwg_last_error
    wide = models.MelGANGenerator(channels=64, upsample_scales=[2, 2], stacks=6, use_causal_conv=True)  # dilation 243
    with pytest.raises(ValueError, match="LDS"):
        CausalStream(wide)


def test_causal_stream_refuses_bf16_precision():
    from parallelwavegan_amd.utils import set_inference_precision

    g = models.HiFiGANGenerator(**synth.HIFIGAN_CAUSAL)
    set_inference_precision(g, "bf16")
    with pytest.raises(ValueError, match="bf16"):
        CausalStream(g)


def _expected_warmup(cfg, melgan):
    """From the configuration alone.  Zero padding needs no input column, a replicated start needs the first one, and
    reflect padding of p = (k - 1) * d columns mirrors columns 1 .. p, i.e. needs the first p + 1.  A layer after
    upsampling by r receives r columns per frame."""
    if not melgan:
        return 1  # HiFi-GAN: ConstantPad1d(0) convolutions and replicate-padded transposed layers only
    need = [((cfg["kernel_size"] - 1) + 1, 1)]  # the reflect-padded input convolution
    rate = 1
    for s in cfg["upsample_scales"]:
        need.append((1, rate))  # transposed layer: one replicated column
        rate *= s
        for j in range(cfg["stacks"]):
            need.append(((cfg["stack_kernel_size"] - 1) * cfg["stack_kernel_size"] ** j + 1, rate))
    need.append(((cfg["kernel_size"] - 1) + 1, rate))  # output convolution
    return max(-(-cols // r) for cols, r in need)


def test_warmup_frames_from_the_geometry():
    g = models.HiFiGANGenerator(**synth.HIFIGAN_CAUSAL)
    m = models.MelGANGenerator(**synth.MELGAN_CAUSAL)
    assert _expected_warmup(synth.HIFIGAN_CAUSAL, False) == 1 and _expected_warmup(synth.MELGAN_CAUSAL, True) == 7
    assert CausalStream.required_warmup_frames(g) == 1
    assert CausalStream.required_warmup_frames(m) == 7  # the k = 7 reflect-padded input convolution dominates
    # a configuration where a dilated stack dominates instead: k = 3 input convolution, stacks up to dilation 27 at rate 2
    cfg = dict(in_channels=80, out_channels=1, kernel_size=3, channels=64, upsample_scales=[2, 2], stack_kernel_size=3,
               stacks=4, use_causal_conv=True)
    assert _expected_warmup(cfg, True) == 28
    assert CausalStream.required_warmup_frames(models.MelGANGenerator(**cfg)) == 28


def test_stream_entry_points_are_exported():
    """The entry points arrived with ABI 14 (tests/test_capi.py keeps header, _lib and library on one version)."""
    assert _lib.ABI_VERSION == _lib.lib().pwg_abi_version() >= 14
    for name in ("pwg_conv1d_stream_supported", "pwg_conv1d_stream_hist_floats", "pwg_conv1d_stream_forward"):
        assert name in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
