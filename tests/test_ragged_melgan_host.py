"""CPU: the host side of ragged MelGAN batches -- the three exported symbols and what they refuse
without a device, the slack / minimum rule of ``MelGANGenerator``, ``MelGANRaggedSynthesizer``'s plan and refusals."""
import ctypes

import pytest
import torch

from parallelwavegan_amd import _lib, layers, ops
from parallelwavegan_amd.models import HiFiGANGenerator, MelGANGenerator, ParallelWaveGANGenerator
from parallelwavegan_amd.utils import MelGANRaggedSynthesizer, RaggedSynthesizer
from tests.golden import synth

# the multi_band_melgan.v2 geometry and an odd-rate one (tests/test_stream_melgan_lookahead_gpu.py)
MB_G = dict(in_channels=80, out_channels=4, kernel_size=7, channels=384, upsample_scales=[8, 4, 2], stack_kernel_size=3,
            stacks=4, use_weight_norm=True, use_causal_conv=False)
TINY_MB = dict(in_channels=80, out_channels=4, kernel_size=7, channels=32, upsample_scales=[3, 2], stack_kernel_size=3,
               stacks=3)


def _last_error():
    return _lib.lib().pwg_last_error().decode()


def _p(addr):
    return ctypes.c_void_p(addr)


def test_symbols_are_exported_and_the_abi_stays():
    lib = _lib.lib()
    for name in ("pwg_mirror_tail", "pwg_resstack_ragged_supported", "pwg_resstack_forward_ragged"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 15 and lib.pwg_abi_version() == 15


def test_mirror_tail_refuses_bad_arguments_without_a_device():
    lib = _lib.lib()
    assert lib.pwg_mirror_tail(None, _p(64), 1, 1, 8, 1, 3, None) != 0 and "NULL" in _last_error()
    assert lib.pwg_mirror_tail(_p(64), None, 1, 1, 8, 1, 3, None) != 0 and "NULL" in _last_error()
    assert lib.pwg_mirror_tail(_p(66), _p(64), 1, 1, 8, 1, 3, None) != 0 and "aligned" in _last_error()
    assert lib.pwg_mirror_tail(_p(64), _p(66), 1, 1, 8, 1, 3, None) != 0 and "aligned" in _last_error()
    for rate in (0, -1):
        assert lib.pwg_mirror_tail(_p(64), _p(64), 1, 1, 8, rate, 3, None) != 0 and f"rate = {rate}" in _last_error()
    assert lib.pwg_mirror_tail(_p(64), _p(64), 1, 1, 8, 1, -1, None) != 0 and "pad = -1" in _last_error()
    for batch, channels, t in ((0, 1, 8), (65536, 1, 8), (1, 0, 8), (1, 1, 0)):
        assert lib.pwg_mirror_tail(_p(64), _p(64), batch, channels, t, 1, 3, None) != 0 and "bad shape" in _last_error()


def test_ragged_stack_refuses_bad_arguments_without_a_device():
    lib = _lib.lib()

    def call(frames, rate, channels=96, t=256, d=3, slope=0.2, x=64, y=128):
        return lib.pwg_resstack_forward_ragged(2, channels, t, d, slope, _p(x), _p(64), None, None, None, _p(y), frames,
                                               rate, None)

    assert call(None, 4) != 0 and "NULL frames" in _last_error()
    assert call(_p(66), 4) != 0 and "4-B aligned" in _last_error()
    for rate in (0, -4, 6):
        assert call(_p(64), rate) != 0 and f"rate = {rate}" in _last_error()
    # ... and everything the plain launch refuses, with its reason, still without a launch
    assert call(_p(64), 4, channels=128) != 0 and "unsupported unit (C=128" in _last_error()
    assert call(_p(64), 4, t=254) != 0 and "unsupported unit" in _last_error() and "T=254" in _last_error()
    assert call(_p(64), 4, d=28) != 0 and "d=28" in _last_error()
    assert call(_p(64), 4, slope=1.5) != 0 and "slope" in _last_error()
    assert call(_p(64), 4, x=128) != 0 and "alias" in _last_error()
    assert call(_p(64), 4, x=0) != 0 and "null pointer" in _last_error()


def test_ragged_stack_supported_is_a_function_of_geometry_and_rate():
    for c in (48, 96, 192):
        for rate in (4, 128):
            assert ops.resstack_ragged_supported(c, 256, 9, rate), (c, rate)
        for rate in (1, 2, 6):
            assert ops.resstack_supported(c, 256, 9) and not ops.resstack_ragged_supported(c, 256, 9, rate), (c, rate)
            assert f"rate = {rate}" in _last_error()
    for rate in (4, 128, 1, 2, 6):
        assert not ops.resstack_ragged_supported(128, 256, 9, rate)
    # what the plain query refuses
    for c, t, d in ((96, 254, 3), (96, 32, 3), (48, 256, 28), (192, 256, 0)):
        assert not ops.resstack_supported(c, t, d) and not ops.resstack_ragged_supported(c, t, d, 4), (c, t, d)


def test_slack_and_minimum_of_the_v2_and_of_a_three_launch_geometry(monkeypatch):
    # v2: scales [8, 4, 2], 4 stacks (dilations 1, 3, 9, 27) of 192 / 96 / 48 channels at rates 8 / 32 / 64: every stack
    # is the one-launch ragged unit and reads no mirror column.  mirror_tail serves the first convolution (padding 3 at
    # rate 1: ceil(3 / 1) = 3 frames) and the last one (padding 3 at rate 64: ceil(3 / 64) = 1): slack 3.
    # min_frames: frames * rate > pad for every reflect-padded layer: 3 // 1 + 1 = 4 (first), 27 // 8 + 1 = 4 (the
    # widest stack at rate 8), 27 // 32 + 1 = 1, 27 // 64 + 1 = 1, 3 // 64 + 1 = 1 (last): 4.
    g = MelGANGenerator(**MB_G)
    assert all(m.ragged_fuses(rate) for m, _, _, rate in g._ragged_walk() if isinstance(m, layers.ResidualStack))
    assert (g.ragged_slack_frames, g.ragged_min_frames) == (3, 4)
    # ... with the unit switched off the 27-dilated convolution at rate 8 reads ceil(27 / 8) = 4 frames of mirror
    with monkeypatch.context() as mp:
        mp.setattr(layers.ResidualStack, "fuse_unit", False)
        assert g.ragged_slack_frames == 4
    # TINY_MB: scales [3, 2], 3 stacks (dilations 1, 3, 9) of 16 / 8 channels at rates 3 / 6: no unit kernel, three
    # launches each.  Slack: first convolution ceil(3 / 1) = 3, stacks at rate 3 ceil(9 / 3) = 3, at rate 6
    # ceil(9 / 6) = 2, last convolution ceil(3 / 6) = 1: 3.  min_frames: 3 // 1 + 1 = 4, 9 // 3 + 1 = 4, 9 // 6 + 1 = 2,
    # 3 // 6 + 1 = 1: 4.
    g = MelGANGenerator(**TINY_MB)
    assert not any(m.ragged_fuses(rate) for m, _, _, rate in g._ragged_walk() if isinstance(m, layers.ResidualStack))
    assert (g.ragged_slack_frames, g.ragged_min_frames) == (3, 4)
    # a wider dilated layer at a low rate decides: scales [2, 2], 4 stacks: dilation 27 at rate 2 -> ceil(27 / 2) = 14
    # frames of slack, 27 // 2 + 1 = 14 frames at least
    g = MelGANGenerator(**dict(TINY_MB, upsample_scales=[2, 2], stacks=4))
    assert (g.ragged_slack_frames, g.ragged_min_frames) == (14, 14)


def test_plan_with_slack_and_minimum():
    lengths = [5, 90, 33, 61, 62, 4, 12]
    plan = RaggedSynthesizer.plan_groups(lengths, max_batch=4, bucket_frames=32, min_frames=4, slack_frames=3)
    assert [g.indices for g in plan.groups] == [(5, 0, 6, 2), (3, 4, 1)]
    assert [g.frames for g in plan.groups] == [(4, 5, 12, 33), (61, 62, 90, 0)]
    # 33 + 3 = 36 -> 64; 90 + 3 = 93 -> 96: t_pad >= max + slack, and 61 + 3 = 64 would still fit a bucket of 64
    assert [g.t_pad for g in plan.groups] == [64, 96]
    for g in plan.groups:
        assert g.t_pad % 32 == 0 and g.t_pad >= max(g.frames) + 3 > g.t_pad - 32
        assert all(n == 0 or 4 <= n <= g.t_pad - 3 for n in g.frames), "what forward_ragged asks of the table"
    assert plan.padded_fraction == pytest.approx(1 - sum(lengths) / (4 * 64 + 4 * 96))
    assert sorted(i for g in plan.groups for i in g.indices) == list(range(len(lengths))), "every input exactly once"
    # the slack moves a length on the bucket boundary into the next bucket
    assert RaggedSynthesizer.plan_groups([64], 1, 32, slack_frames=3).groups[0].t_pad == 96
    assert RaggedSynthesizer.plan_groups([61], 1, 32, slack_frames=3).groups[0].t_pad == 64
    # the defaults are the HiFi-GAN plan
    assert RaggedSynthesizer.plan_groups([64], 1, 32).groups[0].t_pad == 64
    with pytest.raises(ValueError, match=r"MelGANRaggedSynthesizer: item 2 has 3 frames, fewer than reflection can pad \(4\)"):
        RaggedSynthesizer.plan_groups([5, 9, 3], 4, 32, min_frames=4, slack_frames=3, who="MelGANRaggedSynthesizer")
    with pytest.raises(ValueError, match="item 1 is empty"):
        RaggedSynthesizer.plan_groups([5, 0], 4, 32, min_frames=4)
    assert MelGANRaggedSynthesizer.plan_groups is RaggedSynthesizer.plan_groups, "one plan, not a copy"


def test_refused_models_and_cpu_tensors():
    with pytest.raises(ValueError, match="HiFiGANGenerator is not supported.*utils.RaggedSynthesizer"):
        MelGANRaggedSynthesizer(HiFiGANGenerator(**synth.HIFIGAN_TINY))
    with pytest.raises(ValueError, match="ParallelWaveGANGenerator is not supported.*ChunkedSynthesizer"):
        MelGANRaggedSynthesizer(ParallelWaveGANGenerator())
    causal = MelGANGenerator(**synth.MELGAN_CAUSAL)
    with pytest.raises(ValueError, match="causal generator has no ragged forward.*ChunkedSynthesizer"):
        MelGANRaggedSynthesizer(causal)
    with pytest.raises(ValueError, match="causal generator has no ragged forward"):
        causal.forward_ragged(torch.zeros(1, 80, 8), torch.zeros(1, dtype=torch.int32))
    zero_padded = MelGANGenerator(**dict(TINY_MB, out_channels=1, pad="ConstantPad1d", pad_params={"value": 0.0}))
    with pytest.raises(ValueError, match="only a ReflectionPad1d model"):
        zero_padded.forward_ragged(torch.zeros(1, 80, 8), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="only a ReflectionPad1d model.*ChunkedSynthesizer"):
        MelGANRaggedSynthesizer(zero_padded)
    with pytest.raises(ValueError, match="emits 4 channels without a PQMF"):
        MelGANRaggedSynthesizer(MelGANGenerator(**TINY_MB))
    mb = MelGANGenerator(**TINY_MB)
    mb.pqmf = layers.PQMF(subbands=2)
    with pytest.raises(ValueError, match="as many sub-bands as the generator emits"):
        MelGANRaggedSynthesizer(mb)
    g = MelGANGenerator(**dict(TINY_MB, out_channels=1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MelGANRaggedSynthesizer(g)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        g.forward_ragged(torch.zeros(2, 80, 8), torch.tensor([8, 4], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mirror_tail(torch.zeros(2, 3, 8), torch.tensor([8, 3], dtype=torch.int32), 1, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.resstack_forward_ragged(torch.zeros(2, 48, 64), torch.tensor([8, 3], dtype=torch.int32), 4, torch.zeros(8), 1, 0.2)
    # RaggedSynthesizer keeps refusing MelGAN, as before
    with pytest.raises(ValueError, match="MelGANGenerator.*ChunkedSynthesizer"):
        RaggedSynthesizer(MelGANGenerator())
