"""CPU: host logic of the look-ahead stream of the NON-causal HiFi-GAN (utils.LookaheadStream, the delayed form of the
streaming convolution) -- the latencies, the delay plan, what the kernel and the stream refuse, and the
delay rules themselves, emulated in float64 torch against the whole-utterance oracle.  Nothing here launches a kernel."""
import ctypes
import random

import pytest
import torch
import torch.nn.functional as F

from oracle import torch_cpu
from parallelwavegan_amd import _lib, layers, models, ops
from parallelwavegan_amd.layers.causal_conv import lookahead_desc, lookahead_settle_frames, lookahead_state_shapes
from parallelwavegan_amd.utils import LookaheadStream, set_inference_precision
from tests.golden import synth
from tests.util import max_abs, synth_for


def _why():
    return _lib.lib().pwg_last_error().decode()


# ---- latencies and the delay plan ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,latency", [(synth.HIFIGAN_V1, 3258), (synth.HIFIGAN_V1_LIBRITTS, 5687),
                                         (synth.HIFIGAN_TINY, 182)])
def test_latency_from_the_geometry(cfg, latency):
    assert LookaheadStream.latency_samples_of(models.HiFiGANGenerator(**cfg)) == latency


@pytest.mark.parametrize("cfg", [synth.HIFIGAN_V1, synth.HIFIGAN_V1_LIBRITTS, synth.HIFIGAN_TINY,
                                 dict(synth.HIFIGAN_TINY, use_additional_convs=False)])
def test_no_launch_settles_later_than_the_output(cfg):
    """``LookaheadStream`` replays a graph once ``latency_frames`` frames went before a push: its ``settle_frames`` is the
    look-ahead core's degenerate value, which is right because the last launch has the largest delay in frames."""
    g = models.HiFiGANGenerator(**cfg)
    assert lookahead_settle_frames(g.lookahead_plan()) == -(-LookaheadStream.latency_samples_of(g) // g.upsample_factor)


def test_delay_plan_of_the_tiny_config():
    """(rate, delay, delay1, delay2) per launch, by hand from the rules: Conv1d adds its padding, ConvTranspose1d gives
    D * s + s//2 + s%2, the residual of a unit is older by the unit's paddings, the running sum by the difference of the
    block delays (blocks: k 3 x dilations (1, 3) = 6 columns, k 5 x (1, 2) = 10 columns)."""
    def stage(rate, d0):
        return [(rate, d0 + 1, 0, 0), (rate, d0 + 2, 2, 0), (rate, d0 + 5, 0, 0), (rate, d0 + 6, 4, 0),    # k 3: d 1, 3
                (rate, d0 + 2, 0, 0), (rate, d0 + 4, 4, 0), (rate, d0 + 8, 0, 0), (rate, d0 + 10, 6, 4)]  # k 5: d 1, 2

    expected = [(1, 3, 0, 0)]
    expected += [(4, 3 * 4 + 2, 0, 0)] + stage(4, 14)       # up x 4 -> 14, stage -> 24
    expected += [(12, 24 * 3 + 2, 0, 0)] + stage(12, 74)    # up x 3 (odd: padding 2) -> 74, stage -> 84
    expected += [(24, 84 * 2 + 1, 0, 0)] + stage(24, 169)   # up x 2 -> 169, stage -> 179
    expected += [(24, 182, 0, 0)]
    g = models.HiFiGANGenerator(**synth.HIFIGAN_TINY)
    plan = g.lookahead_plan()
    assert [tuple(launch[1:]) for launch in plan] == expected
    assert plan[0].conv is g.input_conv and plan[1].conv is g.upsamples[0][1] and plan[-1].conv is g.output_conv[1]
    # state of one half: per launch its history, then its delay lines
    shapes = lookahead_state_shapes(plan, 2)
    assert shapes[:3] == [(2, 80, 6), (2, 64, 1), (2, 32, 2)]
    assert len(shapes) == len(plan) + sum((launch.delay1 > 0) + (launch.delay2 > 0) for launch in plan)


def test_delay_plan_without_additional_convs():
    g = models.HiFiGANGenerator(**dict(synth.HIFIGAN_TINY, use_additional_convs=False))
    plan = g.lookahead_plan()
    # blocks: k 3 x (1, 3) = 1 + 3 = 4 columns, k 5 x (1, 2) = 2 + 4 = 6 columns; one launch per unit, residual in it
    assert [tuple(launch[1:]) for launch in plan[:6]] == [(1, 3, 0, 0), (4, 14, 0, 0), (4, 15, 1, 0), (4, 18, 3, 0),
                                                        (4, 16, 2, 0), (4, 20, 4, 2)]
    assert plan[-1].delay == (((20 * 3 + 2) + 6) * 2 + 1) + 6 + 3


def test_v1_histories_and_delay_lines_fit_the_kernel():
    for cfg in (synth.HIFIGAN_V1, synth.HIFIGAN_V1_LIBRITTS, synth.HIFIGAN_TINY):
        plan = models.HiFiGANGenerator(**cfg).lookahead_plan()
        for launch in plan:
            for batch, n in ((1, 1), (16, 8)):
                d = lookahead_desc(launch.conv, batch, n)
                assert ops.conv1d_stream_delayed_supported(d, launch.delay1, launch.delay2), (launch, _why())
    v1 = models.HiFiGANGenerator(**synth.HIFIGAN_V1).lookahead_plan()
    assert max(max(launch.delay1, launch.delay2) for launch in v1) == 30
    assert max(shape[-1] for shape in lookahead_state_shapes(v1, 1)) == 50


# ---- the kernel's query --------------------------------------------------------------------------------------------
def test_delayed_supported_answers_without_a_device():
    d = ops.make_conv_desc(2, 24, 40, 9, 9, 5, dilation=3, pad_left=12)
    assert ops.conv1d_stream_delayed_supported(d) and ops.conv1d_stream_delayed_supported(d, 7, 30)
    assert ops.conv1d_stream_delayed_supported(d, 144, 144)
    dt = ops.make_conv_desc(2, 24, 12, 9, 36, 8, stride=4, pad_left=4, transposed=True)
    assert ops.conv1d_stream_delayed_supported(dt, 3, 0)
    assert not ops.conv1d_stream_delayed_supported(d, 145, 0) and "delay" in _why()
    assert not ops.conv1d_stream_delayed_supported(d, 0, 145) and "delay" in _why()
    assert not ops.conv1d_stream_delayed_supported(d, -1, 0) and "negative" in _why()
    for mode in ("reflect", "replicate"):
        dr = ops.make_conv_desc(2, 24, 40, 9, 9, 5, dilation=3, pad_left=12, pad_mode=mode)
        assert ops.conv1d_stream_supported(dr) and not ops.conv1d_stream_delayed_supported(dr) and "pad_mode" in _why()
    # whatever the base geometry refuses, with its reason
    assert not ops.conv1d_stream_delayed_supported(layers.Conv1d(16, 16, 7, padding=3).make_desc(1, 8)) and "causal" in _why()
    assert not ops.conv1d_stream_delayed_supported(ops.make_conv_desc(1, 16, 16, 8, 8, 3, pad_left=2, groups=4))
    assert "groups" in _why()


def test_delayed_entry_points_are_exported_under_the_same_abi():
    assert _lib.ABI_VERSION == _lib.lib().pwg_abi_version() == 15
    for name in ("pwg_conv1d_stream_delayed_supported", "pwg_conv1d_stream_delayed_forward"):
        assert name in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)


def test_delayed_forward_refuses_cpu_tensors():
    d = ops.make_conv_desc(1, 4, 4, 8, 8, 3, pad_left=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.conv1d_stream_delayed_forward(d, torch.zeros(1, 4, 8), None, torch.zeros(1, 4, 2), torch.zeros(3 * 16 * 128))


# ---- what the stream refuses ---------------------------------------------------------------------------------------
def test_lookahead_stream_refuses_models_it_cannot_stream():
    with pytest.raises(ValueError, match="CausalStream"):
        LookaheadStream(models.HiFiGANGenerator(**synth.HIFIGAN_CAUSAL))
    with pytest.raises(ValueError, match="MelGANGenerator"):
        LookaheadStream(models.MelGANGenerator(channels=64, upsample_scales=[4, 2, 2], stacks=2))
    with pytest.raises(ValueError, match="out_channels"):
        LookaheadStream(models.HiFiGANGenerator(**dict(synth.HIFIGAN_TINY, out_channels=4)))
    g = models.HiFiGANGenerator(**synth.HIFIGAN_TINY)
    set_inference_precision(g, "bf16")
    with pytest.raises(ValueError, match="bf16"):
        LookaheadStream(g)
    with pytest.raises(ValueError, match="non-decreasing"):
        LookaheadStream(models.HiFiGANGenerator(**dict(synth.HIFIGAN_TINY, resblock_kernel_sizes=(7, 3))))
    # a history beyond the kernel's cap: (k - 1) * d = 10 * 15 = 150 columns
    with pytest.raises(ValueError, match="LDS"):
        LookaheadStream(models.HiFiGANGenerator(**dict(synth.HIFIGAN_TINY, resblock_kernel_sizes=(11,),
                                                       resblock_dilations=[(1, 15)])))
    with pytest.raises(ValueError, match="batch"):
        LookaheadStream(models.HiFiGANGenerator(**synth.HIFIGAN_TINY), batch=0)


def test_lookahead_stream_on_a_cpu_model_has_no_fallback():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LookaheadStream(models.HiFiGANGenerator(**synth.HIFIGAN_TINY))


def test_causal_generator_has_no_lookahead_plan():
    with pytest.raises(ValueError, match="CausalStream"):
        models.HiFiGANGenerator(**synth.HIFIGAN_CAUSAL).lookahead_plan()


# ---- the rules, emulated -------------------------------------------------------------------------------------------
class LookaheadEmulation:
    """The delay rules of DESIGN.md s11.4 in float64 torch, independent of the package's plan: every layer in causal
    form (``F.conv1d`` over ``concat(history, chunk)``; the full ``F.conv_transpose1d`` cut at ``[s, s + n * s)``), the
    addends through delay lines, zeros stored outside ``[D, D + T * rate)``.  ``sd``: reference-format state dict."""

    def __init__(self, sd, cfg):
        self.sd = {k: v.double() for k, v in sd.items()}
        self.cfg = cfg
        self.state = {}   # name -> history or delay line
        self.cols = {}    # name -> output columns produced so far
        self.up = 1
        for s in cfg["upsample_scales"]:
            self.up *= s
        self.latency = None

    def _line(self, name, new, length):
        """concat(state, new), remembering its last ``length`` columns."""
        b, ch, _ = new.shape
        cat = torch.cat([self.state.get(name, torch.zeros(b, ch, length, dtype=torch.float64)), new], -1)
        self.state[name] = cat[..., cat.shape[-1] - length:]
        return cat

    def _mask(self, name, y, delay, rate, total):
        done = self.cols.get(name, 0)
        tau = torch.arange(done, done + y.shape[-1])
        self.cols[name] = done + y.shape[-1]
        valid = tau >= delay
        if total is not None:
            valid &= tau < delay + total * rate
        return torch.where(valid, y, torch.zeros((), dtype=torch.float64))  # stored zeros, also where y is not finite

    def _conv(self, name, x, d_in, rate, total, dilation=1, slope=None, addends=(), div=1.0, post=None):
        w, b = torch_cpu.get_weight(self.sd, name), torch_cpu.get_bias(self.sd, name)
        reach = (w.shape[-1] - 1) * dilation
        d_out = d_in + reach // 2
        win = self._line(name + ":hist", x, reach)
        y = F.conv1d(win if slope is None else F.leaky_relu(win, slope), w, b, dilation=dilation)
        assert y.shape[-1] == x.shape[-1]
        for i, (a, d_a) in enumerate(addends):
            assert d_out >= d_a
            y = y + self._line(f"{name}:add{i}", a, d_out - d_a)[..., :x.shape[-1]]
        y = y / div
        if post is not None:
            y = post(y)
        return self._mask(name, y, d_out, rate, total), d_out

    def _up(self, name, x, d_in, rate_in, s, slope, total):
        w, b = torch_cpu.get_weight(self.sd, name), torch_cpu.get_bias(self.sd, name)
        d_out = d_in * s + s // 2 + s % 2
        win = self._line(name + ":hist", x, 1)
        n = x.shape[-1]
        y = F.conv_transpose1d(F.leaky_relu(win, slope), w, b, stride=s)[..., s:s + n * s]
        return self._mask(name, y, d_out, rate_in * s, total), d_out

    def push(self, c, total=None):
        """c: (B, C, n) float64 -> (B, n * up): the stream's next columns, still late by ``self.latency``."""
        cfg = self.cfg
        slope = cfg["nonlinear_activation_params"]["negative_slope"]
        x, d = self._conv("input_conv", c, 0, 1, total)
        rate, nb = 1, len(cfg["resblock_kernel_sizes"])
        for i, s in enumerate(cfg["upsample_scales"]):
            x, d0 = self._up(f"upsamples.{i}.1", x, d, rate, s, slope, total)
            rate *= s
            cs = None
            for j, dils in enumerate(cfg["resblock_dilations"]):
                y, dy = x, d0
                for u, dil in enumerate(dils):
                    last = u == len(dils) - 1
                    tail = dict(addends=[(y, dy)] + ([cs] if last and cs is not None else []),
                                div=float(nb) if last and j == nb - 1 else 1.0)
                    p1 = f"blocks.{i * nb + j}.convs1.{u}.1"
                    if cfg["use_additional_convs"]:
                        t, dt = self._conv(p1, y, dy, rate, total, dil, slope)
                        y, dy = self._conv(f"blocks.{i * nb + j}.convs2.{u}.1", t, dt, rate, total, 1, slope, **tail)
                    else:
                        y, dy = self._conv(p1, y, dy, rate, total, dil, slope, **tail)
                cs = (y, dy)
            x, d = cs
        y, self.latency = self._conv("output_conv.1", x, d, rate, total, 1, 0.01, post=torch.tanh)
        return y[:, 0]


def emulate_lookahead(sd, cfg, c, pieces):
    """Whole emulated utterance: ``c`` (B, C, T) in ``pieces``, then ``ceil(latency / up)`` zero frames one at a time
    with the utterance's length known -> (the T * up samples, everything in front of them, everything behind)."""
    em, t, outs = LookaheadEmulation(sd, cfg), 0, []
    total = c.shape[-1]
    for n in pieces:
        outs.append(em.push(c[..., t:t + n].double()))
        t += n
    assert t == total
    for _ in range(-(-em.latency // em.up)):
        outs.append(em.push(torch.zeros(c.shape[0], c.shape[1], 1, dtype=torch.float64), total))
    y = torch.cat(outs, -1)
    return y[:, em.latency:em.latency + total * em.up], y[:, :em.latency], y[:, em.latency + total * em.up:], em.latency


@pytest.mark.parametrize("frames", [1, 23])
@pytest.mark.parametrize("extra", [{}, {"use_additional_convs": False}])
def test_emulated_rules_equal_the_whole_utterance_oracle(frames, extra):
    cfg = dict(synth.HIFIGAN_TINY, **extra)
    g = models.HiFiGANGenerator(**cfg)
    sd = synth_for(g, 21, 1.0)
    c = synth.synth_input("c", (2, 80, frames), seed=21)
    ref = torch_cpu.hifigan_generator({k: v.double() for k, v in sd.items()}, c.double(), **cfg)[:, 0]
    rnd = random.Random(frames)
    pieces = []
    while sum(pieces) < frames:
        pieces.append(rnd.randint(1, min(5, frames - sum(pieces))))
    y, front, back, latency = emulate_lookahead(sd, cfg, c, pieces)
    assert latency == LookaheadStream.latency_samples_of(g)
    assert max_abs(y, ref) < 1e-10
    assert float(front.abs().max()) == 0.0 and float(back.abs().max()) == 0.0  # exact zeros around the utterance
