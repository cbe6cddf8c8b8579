"""CPU: the one walk per module and the one owner of a family's checks -- the causal walk's two
refusals, the single module generator of ``MelGANGenerator`` against what ``forward`` visits and against the rates of
``stream_layers()`` / ``lookahead_plan()``, and the figures of a family's lock-step class against its pool's.  Nothing here
launches a kernel."""
import pytest
import torch

from parallelwavegan_amd import layers, models
from parallelwavegan_amd.layers.causal_conv import (CausalConv1d, CausalConvTranspose1d, CausalWalk, lookahead_settle_frames,
                                                    lookahead_state_shapes, mirrored_min_frames,
                                                    pwg_lookahead_state_shapes)
from parallelwavegan_amd.layers.conv import Conv1d, ConvTranspose1d
from parallelwavegan_amd.utils import (LookaheadStream, MelGANLookaheadStream, MelGANStreamPool, PWGLookaheadStream,
                                       PWGStreamPool, StreamPool)
from tests.golden import synth

MELGAN_TINY = dict(synth.MELGAN_CAUSAL, use_causal_conv=False)
MELGAN_TINY_MB = dict(in_channels=80, out_channels=4, kernel_size=7, channels=32, upsample_scales=[3, 2], stacks=3)
PWG_SMALL = dict(layers=6, stacks=2, aux_context_window=2, upsample_params={"upsample_scales": [4, 4]})


# ---- the causal walk -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls, cfg", [(models.HiFiGANGenerator, synth.HIFIGAN_CAUSAL),
                                      (models.MelGANGenerator, synth.MELGAN_CAUSAL)])
def test_causal_walk_refuses_a_layer_that_is_not_the_next_one(cls, cfg):
    g = cls(**cfg)
    stream_layers = g.stream_layers()
    hist = [torch.zeros(layer.history_shape(1)) for layer, _ in stream_layers]
    x = torch.zeros(1, 80, 4)
    with pytest.raises(RuntimeError, match="causal walk out of step"):  # (raised before anything is launched)
        CausalWalk(stream_layers, None, hist).run(stream_layers[1][0], x)
    walk = CausalWalk(stream_layers, hist, hist)
    assert walk.take(stream_layers[0][0]) == (hist[0], hist[0])
    with pytest.raises(RuntimeError, match="out of step"):
        walk.take(stream_layers[0][0])  # the same layer twice
    done = CausalWalk(stream_layers, None, hist)
    for layer, _ in stream_layers:
        assert done.take(layer)[0] is None  # start of stream: (None, hist_out)
    with pytest.raises(RuntimeError, match="out of step"):
        done.take(stream_layers[-1][0])  # one layer more than stream_layers() has


@pytest.mark.parametrize("cls, cfg", [(models.HiFiGANGenerator, synth.HIFIGAN_CAUSAL),
                                      (models.MelGANGenerator, synth.MELGAN_CAUSAL)])
def test_causal_walk_refuses_history_lists_of_the_wrong_length(cls, cfg):
    g = cls(**cfg)
    stream_layers = g.stream_layers()
    n = len(stream_layers)
    hist = [torch.zeros(layer.history_shape(1)) for layer, _ in stream_layers]
    with pytest.raises(ValueError, match=rf"hist_in / hist_out hold None / {n - 1} history tensors, stream_layers\(\) has {n}"):
        CausalWalk(stream_layers, None, hist[:-1])
    with pytest.raises(ValueError, match=rf"hist_in / hist_out hold {n + 1} / {n} history tensors, stream_layers\(\) has {n}"):
        CausalWalk(stream_layers, hist + hist[:1], hist)
    with pytest.raises(ValueError, match=rf"stream_forward: hist_in / hist_out hold None / 0 history tensors"):
        g.stream_forward(torch.zeros(1, 80, 4), None, [])  # the model's entry point builds the walk


# ---- MelGANGenerator: one generator over self.melgan -----------------------------------------------------------------
COMPUTE = (Conv1d, ConvTranspose1d, CausalConv1d, CausalConvTranspose1d, layers.ResidualStack)


def _visited_by_forward(g):
    """``[(module, keywords)]`` in the order ``forward`` calls the modules of ``g.melgan``, every module stubbed."""
    seen = []
    for m in g.melgan:
        m.forward = lambda x, _m=m, **kw: (seen.append((_m, kw)), x)[1]
    g.forward(torch.zeros(1, 80, 4))
    return seen


@pytest.mark.parametrize("cfg", [synth.MELGAN_CAUSAL, MELGAN_TINY, MELGAN_TINY_MB],
                         ids=["causal", "non_causal", "non_causal_mb"])
def test_melgan_module_generator_is_what_forward_visits(cfg):
    g = models.MelGANGenerator(**cfg)
    stages = list(g._stages())
    want = [m for m in g.melgan if isinstance(m, COMPUTE)]
    assert [m for m, _, _, _ in stages] == want and len(want) == 2 + len(cfg["upsample_scales"]) * (1 + cfg["stacks"])
    assert [last for _, _, last, _ in stages] == [False] * (len(want) - 1) + [True]
    seen = _visited_by_forward(g)
    # (an activation and a pad are visited by nobody: they ride on the next convolution)
    assert [m for m, _ in seen] == want
    slope = cfg.get("nonlinear_activation_params", {"negative_slope": 0.2})["negative_slope"]
    for (m, kw), (_, act, last, _) in zip(seen, stages):
        if isinstance(m, layers.ResidualStack):
            assert kw == {} and act is None
        elif m is want[0]:
            assert kw == {} and act is None
        else:
            assert kw == dict(pre_act="leaky_relu", pre_slope=slope, **({"post_act": "tanh"} if last else {}))
    # the rate of a module's input: the product of the strides in front of it
    rate, rates = 1, []
    for m in want:
        rates.append(rate)
        rate *= m.stride if isinstance(m, (ConvTranspose1d, CausalConvTranspose1d)) else 1
    assert [r for _, _, _, r in stages] == rates and rate == g.upsample_factor


def test_melgan_module_generator_rates_are_those_of_stream_layers_and_the_plan():
    causal = models.MelGANGenerator(**synth.MELGAN_CAUSAL)
    want = []
    for m, _, _, rate in causal._stages():
        want += [(cv, rate) for cv in (m.stream_layers() if isinstance(m, layers.ResidualStack) else [m])]
    assert causal.stream_layers() == want and all(isinstance(cv, (CausalConv1d, CausalConvTranspose1d)) for cv, _ in want)
    for cfg in (MELGAN_TINY, MELGAN_TINY_MB):
        g = models.MelGANGenerator(**cfg)
        plan = iter(g.lookahead_plan())
        for m, _, _, rate in g._stages():
            if isinstance(m, layers.ResidualStack):
                skip, conv0, conv1 = next(plan), next(plan), next(plan)
                assert (skip.conv, conv0.conv, conv1.conv) == (m.skip_layer, m.stack[2], m.stack[4])
                assert skip.rate == conv0.rate == conv1.rate == rate
            else:
                launch = next(plan)
                assert launch.conv is m and launch.rate == rate * (m.stride if m.transposed else 1)
        assert next(plan, None) is None
        assert g._ragged_walk() == list(g._stages())  # 4-tuples, the module first and the rate last


def test_residual_stack_parts_in_either_layout():
    causal, plain = layers.ResidualStack(channels=8, use_causal_conv=True), layers.ResidualStack(channels=8, dilation=3)
    assert causal.parts() == (causal.stack[0], causal.stack[1], causal.stack[2], causal.stack[3], causal.skip_layer)
    assert plain.parts() == (plain.stack[0], plain.stack[2], plain.stack[3], plain.stack[4], plain.skip_layer)
    assert plain.unit_convs() == (plain.stack[2], plain.stack[4], plain.skip_layer)
    assert causal.stream_layers() == [causal.stack[1]] and isinstance(causal.stack[1], CausalConv1d)


# ---- one owner per family: the lock-step class and the pool give the same figures ------------------------------------
def _melgan(cfg):
    g = models.MelGANGenerator(**cfg)
    if cfg["out_channels"] > 1:
        g.pqmf = layers.PQMF(subbands=cfg["out_channels"])
    return g


FAMILIES = {
    "hifigan": (LookaheadStream, StreamPool, lambda: models.HiFiGANGenerator(**synth.HIFIGAN_TINY)),
    "melgan": (MelGANLookaheadStream, MelGANStreamPool, lambda: _melgan(MELGAN_TINY)),
    "mb_melgan": (MelGANLookaheadStream, MelGANStreamPool, lambda: _melgan(MELGAN_TINY_MB)),
    "pwg": (PWGLookaheadStream, PWGStreamPool, lambda: models.ParallelWaveGANGenerator(**PWG_SMALL)),
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_lock_step_class_and_pool_give_the_same_figures(family):
    stream, pool, build = FAMILIES[family]
    g = build()
    plan, pqmf = g.lookahead_plan(), getattr(g, "pqmf", None)
    k = pqmf.subbands if pqmf is not None else 1
    up = g.upsample_factor * k
    latency = (plan[-1].delay + (pqmf.stream_delay_columns if pqmf is not None else 0)) * k
    if family == "pwg":
        shapes, settle, shortest = pwg_lookahead_state_shapes(plan, 3), -(-latency // up), 1
    else:
        shapes = lookahead_state_shapes(plan, 3) + ([pqmf.history_shape(3)] if pqmf is not None else [])
        settle, shortest = max(lookahead_settle_frames(plan), -(-latency // up)), mirrored_min_frames(plan)
    for cls in (stream, pool):
        assert cls.latency_samples_of(g) == latency
        assert cls.settle_frames_of(g) == settle
        assert cls.min_frames_of(g) == shortest
        assert cls.state_bytes_of(g, 3) == 2 * 4 * sum(b * ch * cols for b, ch, cols in shapes)
    # what the constructors build from: the family's refusals (host logic only), then the same figures
    a = stream._streamable(g, 3, None, "fp32")
    b = pool._streamable(g, 3, 5, "fp32")
    assert (a.batch, a.columns, b.batch, b.columns) == (3, 8, 3, 5)
    assert a[2:] == b[2:] == stream._figures_of(g, 3)[2:] == pool._figures_of(g, 3)[2:]
    assert (a.up, a.latency_samples, a.settle_frames, a.min_frames, a.state_shapes) == (up, latency, settle, shortest, shapes)


def test_hifigan_settles_with_its_output():
    """``LookaheadStream.settle_frames`` is ``latency_frames`` and the pool's schedule saturates at the plan's
    ``lookahead_settle_frames``: one figure, since a HiFi-GAN launch is never later, in frames, than the output."""
    for cfg in (synth.HIFIGAN_TINY, dict(synth.HIFIGAN_TINY, use_additional_convs=True), synth.HIFIGAN_V1):
        g = models.HiFiGANGenerator(**cfg)
        latency_frames = -(-g.lookahead_plan()[-1].delay // g.upsample_factor)
        assert StreamPool.settle_frames_of(g) == lookahead_settle_frames(g.lookahead_plan()) == latency_frames
