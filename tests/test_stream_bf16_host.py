"""CPU: host logic of the bf16-operand streaming convolution (pwg_conv1d_stream_bf16_*) and of
``CausalStream(model, precision=...)`` -- coverage equal to the fp32 stream kernel's, the additive ABI, and the
constructor's argument checks.  Nothing here launches a kernel."""
import ctypes
import itertools
import os
import re

import pytest
import torch

from parallelwavegan_amd import _lib, layers, models, ops
from parallelwavegan_amd.utils import CausalStream, set_inference_precision
from tests.golden import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _why():
    return _lib.lib().pwg_last_error().decode()


def _grid():
    """Causal and non-causal convolutions, H of 144 and 146 (and around), grouped, strided, (k, 1) width, the three pad
    modes, every pre-activation, transposed with k == 2s and k != 2s, causal and non-causal transposed padding."""
    out = []
    for pad_mode, pre, (k, d) in itertools.product(("zero", "reflect", "replicate"), (None, "leaky_relu", "relu", "tanh"),
                                                   ((1, 1), (3, 1), (7, 1), (3, 27), (11, 5), (3, 72), (3, 73), (9, 18),
                                                    (74, 2), (2, 144), (2, 146))):
        h = (k - 1) * d
        for c_in, c_out in ((24, 40), (512, 1)):
            out.append((f"causal k{k}d{d} {pad_mode} {pre} {c_in}", ops.make_conv_desc(
                2, c_in, c_out, 9, 9, k, dilation=d, pad_left=h, pad_mode=pad_mode, pre_act=pre, pre_slope=0.1)))
        out.append((f"two-sided k{k}d{d} {pad_mode} {pre}", ops.make_conv_desc(
            1, 16, 16, 40, 40, k, dilation=d, pad_left=h // 2, pad_mode=pad_mode, pre_act=pre)))
    for groups, stride, width in ((4, 1, 1), (1, 2, 1), (1, 1, 3), (16, 1, 1)):
        out.append((f"g{groups} s{stride} w{width}", ops.make_conv_desc(1, 16, 16, 8, 8 // stride, 3, stride=stride, pad_left=2,
                                                                         groups=groups, width=width)))
    for pad_mode, (k, s, p) in itertools.product(("zero", "reflect", "replicate"),
                                                 ((4, 2, 2), (8, 4, 4), (16, 8, 8), (7, 3, 3), (8, 4, 2), (4, 4, 4),
                                                  (16, 8, 4))):
        out.append((f"transposed k{k}s{s}p{p} {pad_mode}", ops.make_conv_desc(
            3, 64, 24, 8, 8 * s, k, stride=s, pad_left=p, transposed=True, pad_mode=pad_mode, pre_act="leaky_relu")))
    out.append(("transposed, wrong t_out", ops.make_conv_desc(1, 64, 24, 8, 30, 8, stride=4, pad_left=4, transposed=True)))
    out.append(("grouped transposed", ops.make_conv_desc(1, 64, 24, 8, 32, 8, stride=4, pad_left=4, groups=2,
                                                         transposed=True)))
    out.append(("batch beyond the grid", ops.make_conv_desc(70000, 8, 8, 4, 4, 3, pad_left=2)))
    out.append(("zero columns", ops.make_conv_desc(1, 8, 8, 0, 0, 3, pad_left=2)))
    for cls, cfg in ((models.HiFiGANGenerator, synth.HIFIGAN_CAUSAL), (models.MelGANGenerator, synth.MELGAN_CAUSAL)):
        for layer, rate in cls(**cfg).stream_layers():
            out.append((f"{cls.__name__} {layer}", layer.stream_desc(2, 8 * rate)))
    return out


def test_bf16_stream_coverage_is_the_fp32_stream_coverage():
    grid = _grid()
    answers = set()
    for name, d in grid:
        fp32 = ops.conv1d_stream_supported(d)
        bf16 = ops.conv1d_stream_bf16_supported(d)
        why = _why()
        assert bf16 == fp32, (name, why)
        assert _lib.lib().pwg_conv1d_stream_bf16_supported(ctypes.byref(d)) in (0, 1)
        if not bf16:
            assert why.strip(), name  # the reason is named
        answers.add(bf16)
    assert answers == {True, False} and len(grid) > 300
    # H = 144 streams, H = 146 does not, in both
    assert ops.conv1d_stream_bf16_supported(ops.make_conv_desc(1, 8, 8, 4, 4, 3, dilation=72, pad_left=144))
    assert not ops.conv1d_stream_bf16_supported(ops.make_conv_desc(1, 8, 8, 4, 4, 3, dilation=73, pad_left=146))
    assert "LDS" in _why()
    assert not ops.conv1d_stream_bf16_supported(ops.make_conv_desc(1, 16, 16, 8, 8, 3, pad_left=2, groups=4))
    assert "groups" in _why()


def test_the_state_of_a_layer_does_not_depend_on_the_precision():
    """One history geometry (pwg_conv1d_stream_hist_floats, history_shape) for both kernels; a reflect-padded layer has a
    bf16 image although the whole-utterance bf16 kernel does not cover it."""
    conv = layers.CausalConv1d(24, 40, 5, dilation=3, pad="ReflectionPad1d", pad_params={})
    d = conv.stream_desc(3, 9)
    assert ops.conv1d_stream_bf16_supported(d) and not ops.conv1d_bf16_supported(d)
    assert ops.conv1d_stream_hist_floats(d) == 3 * 24 * 12 == torch.Size(conv.history_shape(3)).numel()
    zero = ops.ConvDesc.from_buffer_copy(d)
    zero.pad_mode = ops.PAD["zero"]
    assert _lib.lib().pwg_conv1d_bf16_packed_weight_bytes(ctypes.byref(zero)) == 5 * 32 * 64 * 2  # [tap][ci pad 32][m pad 64]


def test_bf16_stream_entry_points_are_additive():
    """Two new symbols, declared, exported and bound; no existing signature changed, so the ABI version stays 15."""
    assert _lib.ABI_VERSION == 15 == _lib.lib().pwg_abi_version()
    header = open(os.path.join(ROOT, "include", "pwg_kernels.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("pwg_conv1d_stream_bf16_supported", "pwg_conv1d_stream_bf16_forward"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["pwg_conv1d_stream_bf16_forward"] == _lib.SIGNATURES["pwg_conv1d_stream_forward"]
    assert "pwg_abi_version() stays 15" in header


def test_bf16_stream_forward_refuses_cpu_tensors_and_bad_precision():
    conv = layers.CausalConv1d(4, 4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv.stream_forward(torch.zeros(1, 4, 8), None, torch.zeros(conv.history_shape(1)), precision="bf16")
    with pytest.raises(ValueError, match="precision"):
        conv.stream_forward(torch.zeros(1, 4, 8), None, torch.zeros(conv.history_shape(1)), precision="int8")
    with pytest.raises(ValueError, match="precision"):
        layers.causal_conv.stream_pointwise(layers.Conv1d(4, 4, 1), torch.zeros(1, 4, 8), precision="fp16")
    # a layer the kernel does not cover: the reason comes from pwg_last_error
    far = layers.CausalConv1d(4, 4, 3, dilation=100)
    with pytest.raises(RuntimeError, match="LDS"):
        far.stream_forward(torch.zeros(1, 4, 8), None, torch.zeros(far.history_shape(1)), precision="bf16")


def test_causal_stream_precision_argument():
    g = models.HiFiGANGenerator(**synth.HIFIGAN_CAUSAL)
    for bad in ("int8", "fp16", "BF16", 16):
        with pytest.raises(ValueError, match="precision"):
            CausalStream(g, precision=bad)
    # a good value passes the argument checks and reaches the device check, on every path
    for ok in (None, "fp32", "bf16"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            CausalStream(g, precision=ok)
    with pytest.raises(ValueError, match="use_causal_conv"):
        CausalStream(models.HiFiGANGenerator(**synth.HIFIGAN_TINY), precision="bf16")
    wide = models.MelGANGenerator(channels=64, upsample_scales=[2, 2], stacks=6, use_causal_conv=True)  # dilation 243
    with pytest.raises(ValueError, match="LDS"):
        CausalStream(wide, precision="bf16")
    # the existing refusal of a bf16-mode model with the default argument (and with "fp32", the same stream) still holds
    set_inference_precision(g, "bf16")
    for default in (None, "fp32"):
        with pytest.raises(ValueError, match="bf16"):
            CausalStream(g, precision=default)
    with pytest.raises(ValueError, match="bf16"):
        CausalStream(g)
    # an explicit bf16 stream does not read the modules' mode: it gets as far as the device check
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CausalStream(g, precision="bf16")
    assert all(cv.precision == "bf16" for cv in layers.conv.each_conv(g) if cv.bf16_capable())
