"""CPU: the host side of ragged Parallel WaveGAN batches -- the three exported symbols and what they
refuse without a device, ``ParallelWaveGANGenerator.ragged_unsupported_reason``, ``PWGRaggedSynthesizer``'s block layout
(the replicated edges), plan, limit and refusals, and the control that shows why a padded batch needs a ragged forward."""
import ctypes

import pytest
import torch

from oracle import torch_cpu
from parallelwavegan_amd import _lib, ops
from parallelwavegan_amd.models import HiFiGANGenerator, MelGANGenerator, ParallelWaveGANGenerator
from parallelwavegan_amd.utils import PWGRaggedSynthesizer, RaggedSynthesizer
from parallelwavegan_amd.utils.streaming import RaggedGroup
from tests.golden import synth
from tests.util import max_abs, synth_for

ALONE_TOL = 2e-5  # the bound of tests/test_ragged_pwg_gpu.py: the ragged forward against the item alone
# (tests/test_pwg_melgan_gpu.py's PWG_G: the v1 generator, here with one stack of 10 layers, dilations 1 .. 512)
PWG_SMALL = dict(in_channels=1, out_channels=1, kernel_size=3, layers=10, stacks=1, residual_channels=64,
                 gate_channels=128, skip_channels=64, aux_channels=80, aux_context_window=2, dropout=0.0,
                 use_weight_norm=True, upsample_net="ConvInUpsampleNetwork",
                 upsample_params={"upsample_scales": [4, 4, 4, 4]})


def _last_error():
    return _lib.lib().pwg_last_error().decode()


def _p(addr):
    return ctypes.c_void_p(addr)


def _desc(**kw):
    args = dict(batch=2, t=1344, dilation=4)
    args.update(kw)
    return ops.make_wavenet_desc(**args)


def test_symbols_are_declared_and_exported_and_the_abi_stays():
    lib = _lib.lib()
    for name in ("pwg_wavenet_layer_ragged_supported", "pwg_wavenet_layer_forward_ragged",
                 "pwg_wavenet_bf16_layer_forward_ragged"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 15 and lib.pwg_abi_version() == 15


def test_ragged_supported_answers_without_a_device_and_names_its_reasons():
    for rate in (4, 256):
        for d in (1, 4, 512):
            assert ops.wavenet_layer_ragged_supported(_desc(dilation=d), rate), (rate, d)
    for rate in (0, -4, 1, 2, 6):
        assert ops.wavenet_layer_supported(_desc()) and not ops.wavenet_layer_ragged_supported(_desc(), rate)
        assert f"rate = {rate}" in _last_error()
    assert not ops.wavenet_layer_ragged_supported(_desc(causal=True), 4) and "causal" in _last_error()
    assert not ops.wavenet_layer_ragged_supported(_desc(aux_channels=40), 4) and "aux_channels = 40" in _last_error()
    assert not ops.wavenet_layer_ragged_supported(_desc(residual_channels=32), 4) and "channels 32" in _last_error()
    assert not ops.wavenet_layer_ragged_supported(_desc(kernel=5), 4) and "kernel 5" in _last_error()
    assert not ops.wavenet_layer_ragged_supported(_desc(batch=0), 4) and "batch = 0" in _last_error()
    assert not ops.wavenet_layer_ragged_supported(_desc(batch=65536), 4) and "batch = 65536" in _last_error()
    assert not ops.wavenet_layer_ragged_supported(_desc(t=0), 4) and "t = 0" in _last_error()
    assert not ops.wavenet_layer_ragged_supported(_desc(dilation=0), 4) and "dilation = 0" in _last_error()
    # the kernel's own limit on t: 32-bit byte offsets into an item of 128 rows
    assert ops.wavenet_layer_ragged_supported(_desc(t=2 ** 23 - 1), 4)
    assert not ops.wavenet_layer_ragged_supported(_desc(t=2 ** 23), 4) and "too long" in _last_error()
    assert not _lib.lib().pwg_wavenet_layer_ragged_supported(None, 4) and "NULL descriptor" in _last_error()
    # whatever the plain query refuses, the ragged one refuses
    for kw in (dict(causal=True), dict(aux_channels=40), dict(t=2 ** 23), dict(batch=0)):
        assert not ops.wavenet_layer_supported(_desc(**kw)) and not ops.wavenet_layer_ragged_supported(_desc(**kw), 4)


@pytest.mark.parametrize("bf16", [False, True])
def test_ragged_forwards_refuse_bad_arguments_without_a_launch(bf16):
    lib = _lib.lib()

    def call(frames=_p(64), rate=4, desc=None, x=64, x_out=128, mfma=32):
        d = ctypes.byref(desc or _desc())
        args = [d, _p(x), _p(64), None, _p(64), None, None, None, _p(x_out), _p(256)]
        if bf16:
            return lib.pwg_wavenet_bf16_layer_forward_ragged(*args, mfma, frames, rate, None)
        return lib.pwg_wavenet_layer_forward_ragged(*args, frames, rate, None)

    assert call(frames=None) != 0 and "NULL frames" in _last_error()
    assert call(frames=_p(66)) != 0 and "4-B aligned" in _last_error()
    for rate in (0, -1, 6):
        assert call(rate=rate) != 0 and f"rate = {rate}" in _last_error()
    assert call(desc=_desc(causal=True)) != 0 and "causal" in _last_error()
    assert call(desc=_desc(aux_channels=40)) != 0 and "aux_channels = 40" in _last_error()
    assert call(x=0) != 0 and "NULL pointer" in _last_error()
    assert call(x=128) != 0 and "alias" in _last_error()
    if bf16:
        assert call(mfma=8) != 0 and "mfma_shape = 8" in _last_error()


def test_ragged_unsupported_reason_of_the_generator():
    assert ParallelWaveGANGenerator().ragged_unsupported_reason() is None  # parallel_wavegan.v1
    assert ParallelWaveGANGenerator().ragged_unsupported_reason("bf16") is None
    assert ParallelWaveGANGenerator(**PWG_SMALL).ragged_unsupported_reason() is None
    assert "precision" in ParallelWaveGANGenerator(**PWG_SMALL).ragged_unsupported_reason("fp16")
    small = dict(PWG_SMALL, layers=4)
    assert "causal" in ParallelWaveGANGenerator(**synth.PWG_CAUSAL).ragged_unsupported_reason()
    no_up = ParallelWaveGANGenerator(**dict(small, upsample_conditional_features=False))
    assert "upsample_conditional_features=False" in no_up.ragged_unsupported_reason()
    assert "MelGANGenerator" in ParallelWaveGANGenerator(**synth.PWG_MELGAN_UPSAMPLER).ragged_unsupported_reason()
    # a block outside the fused geometry
    assert "aux_channels = 40" in ParallelWaveGANGenerator(**dict(small, aux_channels=40)).ragged_unsupported_reason()
    assert "channels 32" in ParallelWaveGANGenerator(**dict(small, residual_channels=32)).ragged_unsupported_reason()
    # a rate the masked stores do not take: 3 * 3 = 9 samples per frame
    odd = ParallelWaveGANGenerator(**dict(small, upsample_params={"upsample_scales": [3, 3]}))
    assert "rate = 9" in odd.ragged_unsupported_reason()
    g = ParallelWaveGANGenerator(**small)
    g.conv_layers[2].fuse_layer = False
    assert "conv_layers[2]: fuse_layer is off" in g.ragged_unsupported_reason()
    g = ParallelWaveGANGenerator(**small)
    g.conv_layers[1].conv.pad_mode = "reflect"
    assert "conv_layers[1]: spectral norm or non-zero padding" in g.ragged_unsupported_reason()
    g = ParallelWaveGANGenerator(**small)
    g.conv_layers[3].conv1x1_skip.precision = "bf16"
    assert "conv_layers[3]: its convolutions are in mixed precision" in g.ragged_unsupported_reason()
    g = ParallelWaveGANGenerator(**dict(small, dropout=0.1))
    assert "dropout in training mode" in g.train().ragged_unsupported_reason()
    assert g.eval().ragged_unsupported_reason() is None
    for kw in (dict(in_channels=2), dict(out_channels=2)):
        assert "one noise row" in ParallelWaveGANGenerator(**dict(small, **kw)).ragged_unsupported_reason()
    # forward_ragged raises that reason, before it looks at a tensor
    with pytest.raises(ValueError, match="forward_ragged: the model is causal"):
        ParallelWaveGANGenerator(**synth.PWG_CAUSAL).forward_ragged(None, None, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ParallelWaveGANGenerator(**small).forward_ragged(torch.zeros(1, 1, 16 * 256), torch.zeros(1, 80, 20),
                                                         torch.zeros(1, dtype=torch.int32))


def test_block_layout_is_the_replicate_padding_of_every_item_alone():
    w, max_batch = 2, 4
    gen = torch.Generator().manual_seed(3)
    feats = [torch.randn(n, 80, generator=gen) for n in (5, 1, 12)]
    plan = PWGRaggedSynthesizer.plan_groups([f.shape[0] for f in feats], max_batch, 4)
    (group,) = plan.groups
    assert group == RaggedGroup((1, 0, 2), (1, 5, 12, 0), 12)
    block = PWGRaggedSynthesizer.block_layout(group, feats, w, max_batch, 80)
    assert block.shape == (max_batch, 12 + 2 * w, 80)
    for j, i in enumerate(group.indices):
        n = feats[i].shape[0]
        # what ``inference`` builds on the item alone, Fn.pad1d(c, w, w, "replicate"), in plain torch
        want = torch.nn.functional.pad(feats[i].t().unsqueeze(0), (w, w), mode="replicate")
        assert torch.equal(block[j, :n + 2 * w].t().unsqueeze(0), want), f"item {i}"
        assert not block[j, n + 2 * w:].any(), f"item {i}: zeros behind the replicated edge"
    assert not block[3].any(), "an unused item holds zeros"
    # no context window: the frames and zeros
    flat = PWGRaggedSynthesizer.block_layout(group, feats, 0, max_batch, 80)
    assert flat.shape == (max_batch, 12, 80) and torch.equal(flat[1, :5], feats[0]) and not flat[1, 5:].any()


def test_plan_and_limits():
    assert PWGRaggedSynthesizer.plan_groups is RaggedSynthesizer.plan_groups, "one plan, not a copy"
    plan = PWGRaggedSynthesizer.plan_groups([40, 3, 90, 20, 64, 31, 10], 4, 32, who="PWGRaggedSynthesizer")
    assert [g.t_pad for g in plan.groups] == [32, 96] and [g.frames for g in plan.groups] == [(3, 10, 20, 31), (40, 64, 90, 0)]
    # max_frames comes from the kernel's limit on a row: 128 * t * 4 < 2^32 at 256 samples per frame
    block = ParallelWaveGANGenerator(**dict(PWG_SMALL, layers=2)).conv_layers[0]
    assert PWGRaggedSynthesizer.kernel_max_columns(block, 256) == 2 ** 23 - 1
    assert (2 ** 23 - 1) // 256 == 32767
    with pytest.raises(ValueError, match=r"PWGRaggedSynthesizer: item 0 has 32768 frames, more than one forward holds \(32767"):
        PWGRaggedSynthesizer.plan_groups([32768], 4, 64, max_frames=32767, who="PWGRaggedSynthesizer")
    assert PWGRaggedSynthesizer.kernel_max_columns(block, 6) == 0, "a rate the kernel does not take holds nothing"


def test_refused_models_and_precisions():
    with pytest.raises(ValueError, match="HiFiGANGenerator is not supported.*utils.RaggedSynthesizer"):
        PWGRaggedSynthesizer(HiFiGANGenerator(**synth.HIFIGAN_TINY))
    with pytest.raises(ValueError, match="MelGANGenerator is not supported.*utils.MelGANRaggedSynthesizer"):
        PWGRaggedSynthesizer(MelGANGenerator())
    with pytest.raises(ValueError, match="no ragged forward: the model is causal.*model.inference.*PWGStream"):
        PWGRaggedSynthesizer(ParallelWaveGANGenerator(**synth.PWG_CAUSAL))
    with pytest.raises(ValueError, match="no ragged forward: upsample_net='MelGANGenerator'.*model.inference"):
        PWGRaggedSynthesizer(ParallelWaveGANGenerator(**synth.PWG_MELGAN_UPSAMPLER))
    g = ParallelWaveGANGenerator(**dict(PWG_SMALL, layers=2))
    with pytest.raises(ValueError, match="precision must be None, 'fp32' or 'bf16', got 'fp16'"):
        PWGRaggedSynthesizer(g, precision="fp16")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PWGRaggedSynthesizer(g)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.wavenet_layer_forward_ragged(_desc(batch=1, t=64), torch.zeros(1, 64, 64), torch.zeros(1, 80, 64), None,
                                         torch.zeros(1, dtype=torch.int32), 4, torch.zeros(8), None, None, None)


def test_control_a_zero_padded_batch_is_not_the_item_alone():
    """Why the ragged forward exists: on the CPU oracle a short item inside a batch padded with zeros (noise and mel zero
    past its replicated edge) differs from the item alone, near its end, by far more than the 2e-5 the ragged forward is
    held to -- the layers past the item's end are not zero where the inputs are (biases, the gate), and the dilated
    taps of the item's last samples read them.  Seed 11, 5 frames inside 12."""
    g = ParallelWaveGANGenerator(**PWG_SMALL)
    sd = synth_for(g, 11, synth.PWG_G_SCALE)
    n, t_pad, w, up = 5, 12, 2, 256
    feat = synth.synth_input("c", (n, 80), seed=11)
    noise = synth.synth_input("z", (n * up,), seed=11)
    group = RaggedGroup((0,), (n,), t_pad)
    c_pad = PWGRaggedSynthesizer.block_layout(group, [feat], w, 1, 80).transpose(1, 2).contiguous()
    z_pad = torch.zeros(1, 1, t_pad * up)
    z_pad[0, 0, :n * up] = noise
    with torch.no_grad():
        alone = torch_cpu.pwg_generator(sd, noise.reshape(1, 1, -1), c_pad[:, :, :n + 2 * w].contiguous(), **PWG_SMALL)
        padded = torch_cpu.pwg_generator(sd, z_pad, c_pad, **PWG_SMALL)[:, :, :n * up]
    near_end = max_abs(padded[:, :, -up:], alone[:, :, -up:])
    print(f"|padded - alone| in the item's last frame: {near_end:.3e}; over the whole item {max_abs(padded, alone):.3e}; "
          f"peak of the item alone {float(alone.abs().max()):.3e}")
    assert near_end > 100 * ALONE_TOL
