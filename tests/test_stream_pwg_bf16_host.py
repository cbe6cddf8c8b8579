"""CPU: host logic of the bf16-operand Parallel WaveGAN streams (utils.PWGStream / utils.PWGLookaheadStream with
``precision="bf16"``, csrc/wavenet_stream_bf16.hip) -- the entry points, the geometry answers (those of
the fp32 forms, word for word), how the stream classes and the block take the precision, and that plan, latency and state
do not depend on it.  Nothing here launches a kernel."""
import ctypes
import os
import re

import pytest
import torch

from parallelwavegan_amd import _lib, layers, models, ops, utils
from parallelwavegan_amd.layers.causal_conv import PWGLookaheadWalk, pwg_lookahead_state_shapes
from parallelwavegan_amd.layers.conv import each_conv
from parallelwavegan_amd.utils import PWGLookaheadStream, PWGStream
from tests.golden import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = dict(layers=6, stacks=2, aux_context_window=2, upsample_params={"upsample_scales": [4, 4]})
DEEP = dict(layers=10, stacks=1, aux_context_window=2, upsample_params={"upsample_scales": [4, 4]})


def _err():
    return _lib.lib().pwg_last_error().decode(errors="replace")


# ---- entry points --------------------------------------------------------------------------------------------------
def test_entry_points_are_additive():
    assert _lib.ABI_VERSION == 15 == _lib.lib().pwg_abi_version()
    header = open(os.path.join(ROOT, "include", "pwg_kernels.h")).read()
    assert "pwg_abi_version() stays 15" in header
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("pwg_wavenet_stream_bf16_supported", "pwg_wavenet_stream_bf16_forward",
                 "pwg_wavenet_stream_bf16_delayed_supported", "pwg_wavenet_stream_bf16_delayed_forward"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    sig = _lib.SIGNATURES
    # the fp32 entries' arguments, then z_out and g_out in front of the stream
    for bf16, fp32 in (("pwg_wavenet_stream_bf16_forward", "pwg_wavenet_stream_forward"),
                       ("pwg_wavenet_stream_bf16_delayed_forward", "pwg_wavenet_stream_delayed_forward")):
        assert sig[bf16][0] == sig[fp32][0]
        assert sig[bf16][1] == sig[fp32][1][:-1] + [ctypes.c_void_p] * 2 + sig[fp32][1][-1:]
    for bf16, fp32 in (("pwg_wavenet_stream_bf16_supported", "pwg_wavenet_stream_supported"),
                       ("pwg_wavenet_stream_bf16_delayed_supported", "pwg_wavenet_stream_delayed_supported")):
        assert sig[bf16] == sig[fp32]
    for name in ("wavenet_stream_bf16_supported", "wavenet_stream_delayed_bf16_supported", "wavenet_stream_forward_bf16",
                 "wavenet_stream_delayed_forward_bf16"):
        assert callable(getattr(ops, name)), name


# ---- geometry answers ----------------------------------------------------------------------------------------------
def test_bf16_layer_geometry_answers_are_the_fp32_ones():
    for d in range(1, 513):
        for batch in (1, 16):
            for n in (1, 63, 64, 1024):
                causal = ops.make_wavenet_desc(batch, n, d, causal=True)
                assert ops.wavenet_stream_bf16_supported(causal), (d, batch, n, _err())
                desc = ops.make_wavenet_desc(batch, n, d)
                for c_delay in (d, 3069):
                    assert ops.wavenet_stream_delayed_bf16_supported(desc, c_delay), (d, batch, n, c_delay, _err())
    bad = [(dict(kernel=5), "kernel"), (dict(residual_channels=32), "channels"), (dict(aux_channels=64), "aux")]
    forms = ((True, ops.wavenet_stream_bf16_supported, ops.wavenet_stream_supported),
             (False, lambda desc: ops.wavenet_stream_delayed_bf16_supported(desc, 2),
              lambda desc: ops.wavenet_stream_delayed_supported(desc, 2)))
    for causal, bf16, fp32 in forms:
        for kw, word in bad + [(dict(causal=not causal), "causal")]:
            desc = ops.make_wavenet_desc(1, 64, 2, **dict(dict(causal=causal), **kw))
            assert not fp32(desc), kw
            reason = _err()
            assert not bf16(desc), kw
            assert word in _err() and _err() == reason, (kw, _err(), reason)
        desc = ops.make_wavenet_desc(0, 64, 2, causal=causal)
        assert not bf16(desc) and "batch" in _err()
    ok = ops.make_wavenet_desc(1, 64, 2)
    assert not ops.wavenet_stream_delayed_bf16_supported(ok, -1) and "negative" in _err()
    assert ops.wavenet_stream_delayed_bf16_supported(ok, 0)
    # byte offsets inside one item's conditioning line are 32-bit
    too_long = 2 ** 31 // (80 * 4) + 1
    assert not ops.wavenet_stream_delayed_supported(ok, too_long)
    reason = _err()
    assert not ops.wavenet_stream_delayed_bf16_supported(ok, too_long) and "too long" in _err() and _err() == reason
    # ... and inside one item's chunk
    long_push = ops.make_wavenet_desc(1, 2 ** 31 // (128 * 4), 2, causal=True)
    assert not ops.wavenet_stream_bf16_supported(long_push) and "too long" in _err()
    # the bf16 packer keeps refusing a causal descriptor: the stream image is packed through a non-causal copy
    assert not ops.wavenet_bf16_supported(ops.make_wavenet_desc(1, 64, 2, causal=True)) and "causal" in _err()


def test_block_reasons_follow_the_precision():
    causal = layers.WaveNetResidualBlock(dilation=2, use_causal_conv=True)
    assert causal.stream_unsupported_reason(2, 7, "bf16") is None
    blk = layers.WaveNetResidualBlock(dilation=2)
    assert blk.lookahead_unsupported_reason(2, 7, 9, "bf16") is None
    assert "negative" in blk.lookahead_unsupported_reason(2, 7, -1, "bf16")
    small = layers.WaveNetResidualBlock(residual_channels=32, gate_channels=64, skip_channels=32)
    assert "channels" in small.lookahead_unsupported_reason(precision="bf16")


# ---- the block's stream calls --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_block_bf16_calls_refuse_only_cpu_tensors(mode):
    """A bf16 call neither reads nor writes the modules' ``precision``: on CPU tensors it gets as far as the device
    check, whether the block is in fp32 or in bf16 mode."""
    x, c = torch.zeros(1, 64, 8), torch.zeros(1, 80, 8)
    h = [torch.zeros(1, 64, 4) for _ in range(2)]
    causal, blk = layers.WaveNetResidualBlock(dilation=2, use_causal_conv=True), layers.WaveNetResidualBlock(dilation=2)
    for b in (causal, blk):
        for cv in b.fused_convs():
            cv.precision = mode
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        causal.stream_forward(x, c, None, h[0], precision="bf16")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        blk.lookahead_forward(x, c, None, 2, (None, h[0]), precision="bf16")
    for b in (causal, blk):
        assert [cv.precision for cv in b.fused_convs()] == [mode] * 4
    # the fp32 call still refuses the bf16 mode, and any other precision is a ValueError
    if mode == "bf16":
        with pytest.raises(RuntimeError, match="bf16"):
            causal.stream_forward(x, c, None, h[0])
        with pytest.raises(RuntimeError, match="bf16"):
            blk.lookahead_forward(x, c, None, 2, (None, h[0]), precision="fp32")
    with pytest.raises(ValueError, match="fp16"):
        causal.stream_forward(x, c, None, h[0], precision="fp16")
    with pytest.raises(ValueError, match="fp16"):
        blk.lookahead_forward(x, c, None, 2, (None, h[0]), precision="fp16")
    # causality is not a precision question
    with pytest.raises(ValueError, match="use_causal_conv"):
        blk.stream_forward(x, c, None, h[0], precision="bf16")
    with pytest.raises(ValueError, match="PWGStream"):
        causal.lookahead_forward(x, c, None, 2, (None, h[0]), precision="bf16")


def test_walk_carries_the_precision():
    plan = models.ParallelWaveGANGenerator(**SMALL).lookahead_plan()
    assert PWGLookaheadWalk(plan, None, []).precision == "fp32"
    assert PWGLookaheadWalk(plan, None, [], precision="bf16").precision == "bf16"
    with pytest.raises(ValueError, match="fp16"):
        PWGLookaheadWalk(plan, None, [], precision="fp16")


# ---- the stream classes ----------------------------------------------------------------------------------------------
STREAMS = [(PWGStream, synth.PWG_CAUSAL), (PWGLookaheadStream, SMALL), (PWGLookaheadStream, {})]


@pytest.mark.parametrize("cls,cfg", STREAMS)
def test_constructor_takes_the_precision(cls, cfg):
    with pytest.raises(ValueError, match="fp16"):
        cls(models.ParallelWaveGANGenerator(**cfg), precision="fp16")
    # a supported model on the CPU gets past every refusal: only the device is missing
    for precision in (None, "fp32", "bf16"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cls(models.ParallelWaveGANGenerator(**cfg), precision=precision)
    # ... in bf16 also when the model was put in bf16 mode, whose attributes stay as they were
    m = models.ParallelWaveGANGenerator(**cfg)
    assert utils.set_inference_precision(m, "bf16") > 0
    before = [cv.precision for cv in each_conv(m)]
    assert "bf16" in before
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cls(m, precision="bf16")
    assert [cv.precision for cv in each_conv(m)] == before
    # the fp32 stream still refuses that model
    for precision in (None, "fp32"):
        with pytest.raises(ValueError, match="bf16"):
            cls(m, precision=precision)


@pytest.mark.parametrize("cls,cfg", STREAMS)
def test_bf16_refusals_name_the_kernels_reason(cls, cfg):
    narrow = dict(cfg, residual_channels=32, gate_channels=64, skip_channels=32)
    with pytest.raises(ValueError, match=r"channels = 32 / 64 / 32"):
        cls(models.ParallelWaveGANGenerator(**narrow), precision="bf16")
    with pytest.raises(ValueError, match="batch"):
        cls(models.ParallelWaveGANGenerator(**cfg), batch=0, precision="bf16")
    with pytest.raises(ValueError, match=r"in_channels / out_channels = 1 / 2"):
        cls(models.ParallelWaveGANGenerator(**dict(cfg, out_channels=2)), precision="bf16")


def test_bf16_streams_keep_refusing_the_other_causality():
    with pytest.raises(ValueError, match="use_causal_conv"):
        PWGStream(models.ParallelWaveGANGenerator(**SMALL), precision="bf16")
    with pytest.raises(ValueError, match="PWGStream"):
        PWGLookaheadStream(models.ParallelWaveGANGenerator(**synth.PWG_CAUSAL), precision="bf16")


@pytest.mark.parametrize("cfg,latency", [({}, 3921), (SMALL, 66), (DEEP, 1075)])
def test_plan_latency_and_state_do_not_depend_on_the_precision(cfg, latency):
    """Host logic only: the model of a bf16 stream (in either mode) has the plan, latency and state shapes of the fp32
    one."""
    m, b = models.ParallelWaveGANGenerator(**cfg), models.ParallelWaveGANGenerator(**cfg)
    utils.set_inference_precision(b, "bf16")
    assert m.lookahead_unsupported_reason(3, "bf16") is None and b.lookahead_unsupported_reason(3, "bf16") is None
    plan, plan_b = m.lookahead_plan(), b.lookahead_plan()
    assert PWGLookaheadStream.latency_samples_of(b) == PWGLookaheadStream.latency_samples_of(m) == latency
    assert [(p.kind, p.rate, p.delay, p.c_delay, list(p.state)) for p in plan] == \
        [(p.kind, p.rate, p.delay, p.c_delay, list(p.state)) for p in plan_b]
    assert pwg_lookahead_state_shapes(plan, 3) == pwg_lookahead_state_shapes(plan_b, 3)


def test_causal_state_does_not_depend_on_the_precision():
    m, b = (models.ParallelWaveGANGenerator(**synth.PWG_CAUSAL) for _ in range(2))
    utils.set_inference_precision(b, "bf16")
    assert m.stream_unsupported_reason(3, "bf16") is None and b.stream_unsupported_reason(3, "bf16") is None
    shapes = [[layer.history_shape(3) for layer, _ in g.stream_layers()] for g in (m, b)]
    assert shapes[0] == shapes[1] and len(shapes[0]) == 3 + 6
    assert [rate for _, rate in m.stream_layers()] == [rate for _, rate in b.stream_layers()]
