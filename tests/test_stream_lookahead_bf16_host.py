"""CPU: host logic of the look-ahead stream with bf16 operands (the delayed form of csrc/conv1d_stream_bf16.hip,
``LookaheadStream(model, precision="bf16")``) -- the two additive entry points, that both precisions
refuse the same descriptors for the same reasons, and what the stream's ``precision`` argument admits.  Nothing here
launches a kernel."""
import ctypes
import itertools

import pytest
import torch

from parallelwavegan_amd import _lib, layers, models, ops
from parallelwavegan_amd.layers.causal_conv import LookaheadWalk
from parallelwavegan_amd.layers.conv import each_conv
from parallelwavegan_amd.utils import LookaheadStream, set_inference_precision
from tests.golden import synth
from tests.test_capi import _declared_symbols

NEW = ("pwg_conv1d_stream_bf16_delayed_supported", "pwg_conv1d_stream_bf16_delayed_forward")


def _why():
    return _lib.lib().pwg_last_error().decode()


# ---- the entry points ----------------------------------------------------------------------------------------------
def test_bf16_delayed_entry_points_are_declared_exported_and_bound():
    assert _lib.ABI_VERSION == _lib.lib().pwg_abi_version() == 15
    declared = _declared_symbols()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    sig = _lib.SIGNATURES
    assert sig["pwg_conv1d_stream_bf16_delayed_forward"] == sig["pwg_conv1d_stream_delayed_forward"]
    assert sig["pwg_conv1d_stream_bf16_delayed_supported"] == sig["pwg_conv1d_stream_delayed_supported"]
    assert callable(ops.conv1d_stream_bf16_delayed_supported) and callable(ops.conv1d_stream_delayed_forward_bf16)


def _descriptors():
    """Plain and transposed layers, every pad_mode; a history of 150 columns; what the base geometry refuses."""
    for mode in ("zero", "reflect", "replicate"):
        yield ops.make_conv_desc(2, 24, 40, 9, 9, 5, dilation=3, pad_left=12, pad_mode=mode)
        yield ops.make_conv_desc(2, 24, 12, 9, 36, 8, stride=4, pad_left=4, transposed=True, pad_mode=mode)
    yield ops.make_conv_desc(1, 32, 32, 8, 8, 11, dilation=15, pad_left=150)             # history beyond the cap
    yield layers.Conv1d(16, 16, 7, padding=3).make_desc(1, 8)                             # not causal
    yield ops.make_conv_desc(1, 16, 16, 8, 8, 3, pad_left=2, groups=4)                    # grouped
    yield ops.make_conv_desc(2, 24, 12, 9, 36, 8, stride=4, pad_left=2, transposed=True)  # transposed, not causal
    yield ops.make_conv_desc(1, 160, 24, 1, 1, 1)                                         # kernel 1: no history


def test_both_precisions_refuse_the_same_descriptors_for_the_same_reasons():
    delays = (0, 7, 144, 145, -1)
    admitted = refused = 0
    for d in _descriptors():
        for d1, d2 in itertools.product(delays, delays):
            fp32 = ops.conv1d_stream_delayed_supported(d, d1, d2)
            why32 = _why()
            bf16 = ops.conv1d_stream_bf16_delayed_supported(d, d1, d2)
            why16 = _why()
            assert bf16 == fp32, (d.kernel, d.pad_mode, d1, d2)
            if fp32:
                admitted += 1
            else:
                refused += 1
                assert why16 == why32 and why16, (d1, d2, why32, why16)
    assert admitted and refused
    # the reasons themselves
    d = ops.make_conv_desc(2, 24, 40, 9, 9, 5, dilation=3, pad_left=12)
    assert ops.conv1d_stream_bf16_delayed_supported(d) and ops.conv1d_stream_bf16_delayed_supported(d, 144, 144)
    assert not ops.conv1d_stream_bf16_delayed_supported(d, 145, 0) and "delay" in _why()
    assert not ops.conv1d_stream_bf16_delayed_supported(d, 0, -1) and "negative" in _why()
    dr = ops.make_conv_desc(2, 24, 40, 9, 9, 5, dilation=3, pad_left=12, pad_mode="reflect")
    assert ops.conv1d_stream_bf16_supported(dr) and not ops.conv1d_stream_bf16_delayed_supported(dr) and "pad_mode" in _why()
    assert not ops.conv1d_stream_bf16_delayed_supported(ops.make_conv_desc(1, 32, 32, 8, 8, 11, dilation=15, pad_left=150))
    assert "LDS" in _why()


def test_bf16_delayed_forward_refuses_cpu_tensors():
    d = ops.make_conv_desc(1, 4, 4, 8, 8, 3, pad_left=2)
    image = torch.zeros(_lib.lib().pwg_conv1d_bf16_packed_weight_bytes(ctypes.byref(d)), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="device image"):
        ops.conv1d_stream_delayed_forward_bf16(d, torch.zeros(1, 4, 8), None, torch.zeros(1, 4, 2), image)


# ---- the stream's precision argument -------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["int8", "fp16", "BF16", 16])
def test_lookahead_stream_refuses_other_precisions(precision):
    with pytest.raises(ValueError, match="precision"):
        LookaheadStream(models.HiFiGANGenerator(**synth.HIFIGAN_TINY), precision=precision)
    with pytest.raises(ValueError, match="precision"):
        LookaheadWalk([], None, [], precision=precision)


@pytest.mark.parametrize("precision", [None, "fp32", "bf16"])
def test_lookahead_stream_on_a_cpu_model_has_no_fallback(precision):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LookaheadStream(models.HiFiGANGenerator(**synth.HIFIGAN_TINY), precision=precision)


def test_a_bf16_mode_model_is_refused_in_fp32_and_admitted_in_bf16():
    g = models.HiFiGANGenerator(**synth.HIFIGAN_TINY)
    set_inference_precision(g, "bf16")
    for precision in (None, "fp32"):
        with pytest.raises(ValueError, match="bf16") as info:
            LookaheadStream(g, precision=precision)
        assert "precision='bf16'" in str(info.value)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # (past every check of the model: the device check)
        LookaheadStream(g, precision="bf16")
    assert all(cv.precision == "bf16" for cv in each_conv(g))  # neither read nor written


def test_the_model_refusals_still_fire_with_bf16():
    with pytest.raises(ValueError, match="CausalStream"):
        LookaheadStream(models.HiFiGANGenerator(**synth.HIFIGAN_CAUSAL), precision="bf16")
    with pytest.raises(ValueError, match="MelGANGenerator"):
        LookaheadStream(models.MelGANGenerator(channels=64, upsample_scales=[4, 2, 2], stacks=2), precision="bf16")
    with pytest.raises(ValueError, match="out_channels"):
        LookaheadStream(models.HiFiGANGenerator(**dict(synth.HIFIGAN_TINY, out_channels=4)), precision="bf16")
    with pytest.raises(ValueError, match="non-decreasing"):
        LookaheadStream(models.HiFiGANGenerator(**dict(synth.HIFIGAN_TINY, resblock_kernel_sizes=(7, 3))), precision="bf16")
    with pytest.raises(ValueError, match="LDS"):
        LookaheadStream(models.HiFiGANGenerator(**dict(synth.HIFIGAN_TINY, resblock_kernel_sizes=(11,),
                                                       resblock_dilations=[(1, 15)])), precision="bf16")
    with pytest.raises(ValueError, match="batch"):
        LookaheadStream(models.HiFiGANGenerator(**synth.HIFIGAN_TINY), batch=0, precision="bf16")
