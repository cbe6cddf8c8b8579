"""CPU: host side of the opt-in bf16-operand inference mode (no GPU needed)."""
import pytest
import torch

from oracle import torch_cpu
from parallelwavegan_amd import _lib, ops
from parallelwavegan_amd.layers.conv import _ConvNd
from parallelwavegan_amd.models import HiFiGANGenerator, HiFiGANMultiScaleMultiPeriodDiscriminator
from parallelwavegan_amd.utils import get_inference_precision, set_inference_precision
from tests.bf16_emulation import bf16_operands
from tests.golden import synth
from tests.util import synth_for


def _convs(model):
    return [m for m in model.modules() if isinstance(m, _ConvNd)]


@pytest.mark.parametrize("name", ["HIFIGAN_V1", "HIFIGAN_V1_LIBRITTS", "HIFIGAN_TINY"])
def test_every_generator_convolution_is_supported(name):
    g = HiFiGANGenerator(**getattr(synth, name))
    convs = _convs(g)
    assert len(convs) >= 10
    for m in convs:  # support is a matter of geometry, not of length or batch: walk a few of each
        for batch, length in ((1, 1), (2, 7), (3, 96), (16, 10405)):
            d = m.make_desc(batch, length, pre_act="leaky_relu", pre_slope=0.1, post_act="tanh", out_div=3.0)
            assert ops.conv1d_bf16_supported(d), (name, m, _lib.lib().pwg_last_error())
    assert all(m.bf16_capable() for m in convs)


@pytest.mark.parametrize("kwargs,reason", [
    (dict(groups=4), b"groups"),
    (dict(width=3), b"width"),
    (dict(pad_mode="reflect"), b"padding"),
])
def test_unsupported_descriptors_name_the_reason(kwargs, reason):
    d = ops.make_conv_desc(2, 32, 32, 64, 64, 3, pad_left=1, **kwargs)
    assert not ops.conv1d_bf16_supported(d)
    assert reason in _lib.lib().pwg_last_error()
    assert _lib.lib().pwg_conv1d_bf16_packed_weight_bytes(d) == 0
    # further limits of the kernel: strided Conv1d, transposed with k != 2 s
    assert not ops.conv1d_bf16_supported(ops.make_conv_desc(1, 32, 32, 64, 32, 4, stride=2, pad_left=1))
    assert b"stride" in _lib.lib().pwg_last_error()
    assert not ops.conv1d_bf16_supported(ops.make_conv_desc(1, 32, 32, 8, 24, 5, stride=3, pad_left=1, transposed=True))


def test_packed_weight_bytes():
    import ctypes

    n = _lib.lib().pwg_conv1d_bf16_packed_weight_bytes
    # [tap][c_in padded to 32][rows padded to the row tile] bf16
    assert n(ctypes.byref(ops.make_conv_desc(1, 80, 512, 32, 32, 7, pad_left=3))) == 7 * 96 * 512 * 2
    assert n(ctypes.byref(ops.make_conv_desc(1, 32, 1, 32, 32, 7, pad_left=3))) == 7 * 32 * 32 * 2
    assert n(ctypes.byref(ops.make_conv_desc(1, 512, 256, 32, 256, 16, stride=8, pad_left=4, transposed=True))) \
        == 2 * 512 * (8 * 256) * 2


def test_emulation_is_identity_when_the_predicate_says_no_and_rounds_when_it_says_yes():
    cfg = synth.HIFIGAN_TINY
    g = HiFiGANGenerator(**cfg)
    sd = synth_for(g, 5, 1.25)
    c = synth.synth_input("c", (2, 80, 9), seed=9)
    with torch.no_grad():
        ref = torch_cpu.hifigan_generator(sd, c, **cfg)
        with bf16_operands(lambda kind, x, w, kw: False) as st_no:
            no = torch_cpu.hifigan_generator(sd, c, **cfg)
        with bf16_operands() as st_yes:
            yes = torch_cpu.hifigan_generator(sd, c, **cfg)
        with bf16_operands(lambda kind, x, w, kw: kind == "conv_transpose1d") as st_mixed:
            mixed = torch_cpu.hifigan_generator(sd, c, **cfg)
        again = torch_cpu.hifigan_generator(sd, c, **cfg)  # the wrappers are gone
    n_conv = len(_convs(g))
    assert st_no == {"rounded": 0, "untouched": n_conv}
    assert st_yes == {"rounded": n_conv, "untouched": 0}
    assert st_mixed == {"rounded": len(cfg["upsample_scales"]), "untouched": n_conv - len(cfg["upsample_scales"])}
    assert torch.equal(no, ref) and torch.equal(again, ref)
    assert not torch.equal(yes, ref) and not torch.equal(mixed, ref) and not torch.equal(mixed, yes)
    # the rounding is small against the signal (bf16 has 8 significant bits)
    assert (yes - ref).pow(2).mean().sqrt() < 0.05 * ref.pow(2).mean().sqrt()


def test_set_inference_precision_counts_and_restores():
    g = HiFiGANGenerator(**synth.HIFIGAN_V1)
    convs = _convs(g)
    assert len(convs) == 1 + 4 + 12 * 6 + 1
    assert all(m.precision == "fp32" for m in convs) and get_inference_precision(g) == "fp32"
    assert set_inference_precision(g, "bf16") == len(convs)
    assert all(m.precision == "bf16" for m in convs) and get_inference_precision(g) == "bf16"
    assert "precision" not in "".join(g.state_dict().keys())  # a module attribute, not state
    assert set_inference_precision(g, "fp32") == len(convs)
    assert all(m.precision == "fp32" for m in convs) and get_inference_precision(g) == "fp32"
    with pytest.raises(ValueError):
        set_inference_precision(g, "fp16")


def test_uncovered_convolutions_stay_fp32():
    """Grouped and (k, 1) convolutions are outside the bf16 kernel: they keep the fp32 kernels and are not counted."""
    d = HiFiGANMultiScaleMultiPeriodDiscriminator()
    convs = _convs(d)
    n = set_inference_precision(d, "bf16")
    took = [m for m in convs if m.precision == "bf16"]
    assert n == len(took) and 0 < n < len(convs)
    for m in convs:
        assert (m.precision == "bf16") == (m.groups == 1 and not m.width_mode and m.stride == 1 and m.pad_mode == "zero")
    assert set_inference_precision(d, "fp32") == len(convs)


def test_bf16_mode_needs_no_gradient():
    """The gradient check sits in front of any device work: it raises on the host."""
    g = HiFiGANGenerator(**synth.HIFIGAN_TINY)
    set_inference_precision(g, "bf16")
    with pytest.raises(RuntimeError, match="bf16 inference precision"):
        g(torch.zeros(1, 80, 4))
