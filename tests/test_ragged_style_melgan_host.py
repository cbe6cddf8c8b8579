"""CPU: the host side of ragged StyleMelGAN batches -- the four exported symbols and what they and their
wrappers refuse without a device, ``StyleMelGANRaggedSynthesizer``'s plan in noise segments, block layout (the last frame
replicated to the segment boundary), refusals and noise checks, and the float64 proof of the rule the kernels implement:
statistics over the item alone and zeros past its end behind every layer give each item what it gives alone."""
import ctypes

import pytest
import torch

from oracle import torch_cpu
from parallelwavegan_amd import _lib, ops
from parallelwavegan_amd.models import (HiFiGANGenerator, MelGANGenerator, ParallelWaveGANGenerator,
                                        StyleMelGANGenerator)
from parallelwavegan_amd.utils import RaggedSynthesizer, StyleMelGANRaggedSynthesizer
from parallelwavegan_amd.utils.streaming import RaggedGroup
from tests import style_melgan_ragged_refs as refs
from tests.golden import synth
from tests.util import max_abs, synth_for

SYMBOLS = ("pwg_instance_norm_ragged", "pwg_upsample_nearest_ragged", "pwg_tade_modulate_ragged",
           "pwg_softmax_gate_ragged")


def _last_error():
    return _lib.lib().pwg_last_error().decode()


def _p(addr):
    return ctypes.c_void_p(addr)


def test_symbols_are_declared_and_exported_and_the_abi_stays():
    lib = _lib.lib()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 15 and lib.pwg_abi_version() == 15


def test_entry_points_refuse_bad_arguments_without_a_launch():
    lib = _lib.lib()
    calls = {
        "instance_norm_ragged": lambda x=64, y=128, fr=256, b=2, c=3, t=8, rate=1: lib.pwg_instance_norm_ragged(
            _p(x), _p(y), _p(fr), b, c, t, rate, 1e-5, None),
        "upsample_nearest_ragged": lambda x=64, y=128, fr=256, b=2, c=3, t=8, rate=1: lib.pwg_upsample_nearest_ragged(
            _p(x), None, _p(y), _p(fr), b, c, t, 2, rate, None),
        "tade_modulate_ragged": lambda x=64, y=128, fr=256, b=2, c=3, t=8, rate=1: lib.pwg_tade_modulate_ragged(
            _p(x), _p(512), _p(y), _p(fr), b, c, t, 2, rate, None),
        "softmax_gate_ragged": lambda x=64, y=128, fr=256, b=2, c=3, t=8, rate=1: lib.pwg_softmax_gate_ragged(
            _p(x), _p(y), _p(fr), b, c, t, rate, 1, None),
    }
    for name, call in calls.items():
        assert call(x=0) != 0 and f"{name}: NULL pointer" in _last_error()
        assert call(y=0) != 0 and f"{name}: NULL pointer" in _last_error()
        assert call(fr=0) != 0 and f"{name}: NULL pointer" in _last_error()
        assert call(x=66) != 0 and "4-B aligned" in _last_error()
        assert call(fr=258) != 0 and "4-B aligned" in _last_error()
        for rate in (0, -2):
            assert call(rate=rate) != 0 and f"{name}: rate = {rate}" in _last_error()
        for b in (0, 65536):
            assert call(b=b) != 0 and f"batch {b}" in _last_error()
        assert call(c=0) != 0 and "channels 0" in _last_error()
        assert call(t=0) != 0 and "bad shape" in _last_error()
    assert lib.pwg_upsample_nearest_ragged(_p(64), None, _p(128), _p(256), 1, 1, 2 ** 30, 2, 1, None) != 0
    assert "bad shape" in _last_error()
    assert lib.pwg_tade_modulate_ragged(_p(64), _p(512), _p(128), _p(256), 1, 1, 8, 0, 1, None) != 0
    assert "scale 0" in _last_error()


def test_wrappers_refuse_cpu_tensors():
    frames = torch.zeros(2, dtype=torch.int32)
    x, cg = torch.zeros(2, 3, 8), torch.zeros(2, 6, 8)
    for call in (lambda: ops.instance_norm_ragged(x, frames, 1),
                 lambda: ops.upsample_nearest_ragged(x, 2, frames, 2),
                 lambda: ops.tade_modulate_ragged(x, cg, 1, frames, 1),
                 lambda: ops.softmax_gate_ragged(cg, True, frames, 1)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    g = StyleMelGANGenerator(**synth.STYLE_MELGAN_TINY)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        g.forward_ragged(torch.zeros(2, 80, 8), torch.zeros(2, 16, 2), frames)
    with pytest.raises(ValueError, match=r"2 noise columns take 8 frames \(noise_upsample_factor = 4\), got 9"):
        g.forward_ragged(torch.zeros(2, 80, 9), torch.zeros(2, 16, 2), frames)
    with pytest.raises(ValueError, match=r"expected \(B, aux_channels, S_max \* 4\) features"):
        g.forward_ragged(torch.zeros(80, 8), torch.zeros(2, 16, 2), frames)
    with pytest.raises(ValueError, match=r"expected \(B, aux_channels, S_max \* 4\) features"):
        g.forward_ragged(torch.zeros(2, 80, 8), torch.zeros(16, 2), frames)


def test_the_plan_works_in_segments():
    plan = StyleMelGANRaggedSynthesizer.plan_segments
    assert StyleMelGANRaggedSynthesizer.plan_groups is RaggedSynthesizer.plan_groups, "one plan, not a copy"
    # F = 88: 200 .. 800 frames are 3 .. 10 segments
    lengths = [200, 800, 88, 89, 440, 1, 176]
    p = plan(lengths, 88, max_batch=4, bucket_segments=2)
    assert [g.indices for g in p.groups] == [(2, 5, 3, 6), (0, 4, 1)]
    assert [g.frames for g in p.groups] == [(1, 1, 2, 2), (3, 5, 10, 0)]
    assert [g.t_pad for g in p.groups] == [2, 10]
    assert p.padded_fraction == pytest.approx(1.0 - 24 / (4 * 2 + 4 * 10))
    # bucket_segments rounds S_pad up
    assert [g.t_pad for g in plan([89, 400], 88, 4, 4).groups] == [8]
    assert plan([3, 19, 7, 12], 4, 5, 1).groups == [RaggedGroup((0, 2, 3, 1), (1, 2, 3, 5, 0), 5)]
    with pytest.raises(ValueError, match=r"StyleMelGANRaggedSynthesizer: item 1 is empty \(0 frames\)"):
        plan([5, 0], 88)
    with pytest.raises(ValueError, match=r"StyleMelGANRaggedSynthesizer: item 0 has 65536 frames, more than one forward "
                                         r"holds \(65535"):
        plan([65536], 88, max_frames=65535)
    # max_frames of the default generator: 2 * 64 rows x 256 samples per frame in 32-bit element counts
    assert (2 ** 31 - 1) // (2 * 64 * 256) == 65535


def test_block_layout_replicates_the_last_frame_to_the_segment_boundary():
    F, max_batch = 4, 5
    gen = torch.Generator().manual_seed(3)
    feats = [torch.randn(n, 80, generator=gen) for n in (19, 7, 12, 3)]
    (group,) = StyleMelGANRaggedSynthesizer.plan_segments([f.shape[0] for f in feats], F, max_batch, 2).groups
    assert group == RaggedGroup((3, 1, 2, 0), (1, 2, 3, 5, 0), 6)
    block = StyleMelGANRaggedSynthesizer.block_layout(group, feats, F, max_batch, 80)
    assert block.shape == (max_batch, 6 * F, 80)
    for j, i in enumerate(group.indices):
        n, s = feats[i].shape[0], group.frames[j]
        # what ``inference`` builds on the item alone, Fn.pad1d(c, 0, s * F - n, "replicate"), in plain torch
        want = torch.nn.functional.pad(feats[i].t().unsqueeze(0), (0, s * F - n), mode="replicate")
        assert torch.equal(block[j, :s * F].t().unsqueeze(0), want), f"item {i}"
        assert not block[j, s * F:].any(), f"item {i}: zeros behind the segment boundary"
    assert not block[4].any(), "an unused item holds zeros"


def test_refused_models():
    with pytest.raises(ValueError, match="HiFiGANGenerator is not supported.*only StyleMelGANGenerator.*"
                                         "utils.RaggedSynthesizer batches"):
        StyleMelGANRaggedSynthesizer(HiFiGANGenerator(**synth.HIFIGAN_TINY))
    with pytest.raises(ValueError, match="MelGANGenerator is not supported.*utils.MelGANRaggedSynthesizer batches"):
        StyleMelGANRaggedSynthesizer(MelGANGenerator())
    with pytest.raises(ValueError, match="ParallelWaveGANGenerator is not supported.*utils.PWGRaggedSynthesizer batches"):
        StyleMelGANRaggedSynthesizer(ParallelWaveGANGenerator(layers=2, stacks=1))
    with pytest.raises(ValueError, match="Linear is not supported.*utils.ChunkedSynthesizer"):
        StyleMelGANRaggedSynthesizer(torch.nn.Linear(2, 2))
    two = StyleMelGANGenerator(**dict(synth.STYLE_MELGAN_TINY, out_channels=2))
    with pytest.raises(ValueError, match="emits 2 channels; an item returns one waveform.*utils.ChunkedSynthesizer"):
        StyleMelGANRaggedSynthesizer(two)
    g = StyleMelGANGenerator(**synth.STYLE_MELGAN_TINY)
    with pytest.raises(ValueError, match="max_batch and bucket_segments must be >= 1"):
        StyleMelGANRaggedSynthesizer(g, bucket_segments=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        StyleMelGANRaggedSynthesizer(g)


def test_noise_errors_name_the_item():
    s = StyleMelGANRaggedSynthesizer.__new__(StyleMelGANRaggedSynthesizer)  # (the check is host logic of two fields)
    s.segment_frames, s.noise_channels = 4, 16
    feats = [torch.zeros(19, 80), torch.zeros(7, 80)]
    good = [torch.zeros(16, 5), torch.zeros(16, 2)]
    assert [tuple(z.shape) for z in s._checked_noises(feats, good)] == [(16, 5), (16, 2)]
    assert [tuple(z.shape) for z in s._checked_noises(feats, None)] == [(16, 5), (16, 2)]
    with pytest.raises(ValueError, match="1 noises for 2 utterances"):
        s._checked_noises(feats, good[:1])
    with pytest.raises(ValueError, match=r"item 1: expected \(16, 2\) noise for 7 frames, got \(16, 3\)"):
        s._checked_noises(feats, [good[0], torch.zeros(16, 3)])
    with pytest.raises(ValueError, match=r"item 0: expected \(16, 5\) noise for 19 frames, got \(5, 16\)"):
        s._checked_noises(feats, [torch.zeros(5, 16), good[1]])
    # the host draw is inference's own call, per utterance in input order
    torch.manual_seed(5)
    drawn = s._checked_noises(feats, None)
    torch.manual_seed(5)
    for f, z in zip(feats, drawn):
        assert torch.equal(z, torch.randn(1, 16, (f.shape[0] - 1) // 4 + 1, dtype=torch.float)[0])


@pytest.mark.parametrize("name", ["STYLE_MELGAN_TINY", "STYLE_MELGAN_TINY_SIGMOID"])
def test_the_rule_in_float64_is_every_item_alone(name):
    """Statistics over [0, e) and zeros past e behind every layer: in float64 the padded batch gives every item what
    the oracle gives on the item alone (its last frame replicated to the segment boundary) to rounding, and exact zeros
    behind -- whatever the inputs hold past the items' ends."""
    cfg = getattr(synth, name)
    F = 4
    sd = {k: v.double() for k, v in synth_for(StyleMelGANGenerator(**cfg), refs.SEED, refs.G_SCALE).items()}
    its = [(f.double(), z.double()) for f, z in refs.items(cfg)]
    segments = refs.segments_of(refs.FRAMES, F)
    assert segments == (5, 2, 3, 1, 0)
    c, z = refs.padded_batch(its, F, 5, fill=1e3)
    c, z = c.double(), z.double()
    with torch.no_grad():
        y = refs.ragged_generator(sd, c, z, segments, **cfg)
        assert y.shape == (5, 1, 5 * F * 8)
        for j, ((feat, noise), s) in enumerate(zip(its, segments)):
            e = s * F * 8
            assert not y[j, :, e:].any(), f"item {j}: not zero past its end"
            if s:
                alone = torch_cpu.style_melgan_generator(sd, *refs.alone_inputs(feat, noise, F), **cfg)
                err = max_abs(y[j:j + 1, :, :e], alone)
                print(f"{name} item {j} ({feat.shape[0]} frames, {s} segments): |rule - oracle alone| {err:.3e}, peak "
                      f"{float(alone.abs().max()):.3e}")
                assert err < 1e-10, f"item {j}"
