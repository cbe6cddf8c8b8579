"""CPU: host logic of the look-ahead stream of the NON-causal Parallel WaveGAN (utils.PWGLookaheadStream, the delayed
form of csrc/wavenet_stream.hip, pwg_stretch_conv_stream_delayed, pwg_delay_line_forward) -- the
entry points, the geometry answers, the latencies, the plan, what the stream refuses, and the delay rules themselves,
emulated in float64 torch against the whole-utterance oracle.  Nothing here launches a kernel."""
import ctypes
import math
import os
import random
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import torch_cpu
from parallelwavegan_amd import _lib, layers, models, ops, utils
from parallelwavegan_amd.layers.causal_conv import pwg_lookahead_state_shapes
from parallelwavegan_amd.utils import PWGLookaheadStream
from tests.golden import synth
from tests.util import max_abs, synth_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = dict(layers=6, stacks=2, aux_context_window=2, upsample_params={"upsample_scales": [4, 4]})   # 52 + 14
DEEP = dict(layers=10, stacks=1, aux_context_window=2, upsample_params={"upsample_scales": [4, 4]})   # 52 + 1023


def _err():
    return _lib.lib().pwg_last_error().decode(errors="replace")


# ---- entry points --------------------------------------------------------------------------------------------------
def test_entry_points_are_additive():
    assert _lib.ABI_VERSION == 15 == _lib.lib().pwg_abi_version()
    header = open(os.path.join(ROOT, "include", "pwg_kernels.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for ret, name in (("int", "pwg_wavenet_stream_delayed_supported"), ("size_t", "pwg_wavenet_stream_delayed_hist_floats"),
                      ("int", "pwg_wavenet_stream_delayed_forward"), ("int", "pwg_stretch_conv_stream_delayed"),
                      ("int", "pwg_delay_line_forward")):
        assert re.search(r"\b" + ret + " " + name + r"\(", header), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    for name in ("wavenet_stream_delayed_supported", "wavenet_stream_delayed_hist_floats", "wavenet_stream_delayed_forward",
                 "stretch_conv_stream_delayed", "delay_line_forward"):
        assert callable(getattr(ops, name)), name
    assert PWGLookaheadStream is utils.PWGLookaheadStream


# ---- geometry answers ----------------------------------------------------------------------------------------------
def test_delayed_layer_geometry_answers_without_a_gpu():
    for d in range(1, 513):
        for batch in (1, 16):
            for n in (1, 63, 64, 1024):
                desc = ops.make_wavenet_desc(batch, n, d)
                for c_delay in (d, 3069):
                    assert ops.wavenet_stream_delayed_supported(desc, c_delay), (d, batch, n, c_delay, _err())
                assert ops.wavenet_stream_delayed_hist_floats(desc) == batch * 64 * 2 * d
    bad = [(dict(causal=True), "causal"), (dict(kernel=5), "kernel"), (dict(residual_channels=32), "channels"),
           (dict(aux_channels=64), "aux")]
    for kw, word in bad:
        desc = ops.make_wavenet_desc(1, 64, 2, **kw)
        assert not ops.wavenet_stream_delayed_supported(desc, 2), kw
        assert word in _err(), (kw, _err())
        assert ops.wavenet_stream_delayed_hist_floats(desc) == 0
    desc = ops.make_wavenet_desc(0, 64, 2)
    assert not ops.wavenet_stream_delayed_supported(desc, 2) and "batch" in _err()
    assert ops.wavenet_stream_delayed_hist_floats(desc) == 0
    ok = ops.make_wavenet_desc(1, 64, 2)
    assert not ops.wavenet_stream_delayed_supported(ok, -1) and "negative" in _err()
    assert ops.wavenet_stream_delayed_supported(ok, 0)
    # byte offsets inside one item's conditioning line are 32-bit
    assert not ops.wavenet_stream_delayed_supported(ok, 2 ** 31 // (80 * 4) + 1) and "too long" in _err()
    # the causal entry still refuses the non-causal descriptor
    assert not ops.wavenet_stream_supported(ok) and "causal" in _err()


def test_delayed_launches_refuse_cpu_tensors():
    blk = layers.WaveNetResidualBlock(dilation=2)
    x, c = torch.zeros(1, 64, 8), torch.zeros(1, 80, 8)
    h = [torch.zeros(1, 64, 4) for _ in range(2)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        blk.lookahead_forward(x, c, None, 2, (None, h[0]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.stretch_conv_stream_delayed(c, None, torch.zeros(1, 80, 2), torch.zeros(9), 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.delay_line_forward(c, None, torch.zeros(1, 80, 5))


def test_block_lookahead_forward_refusals():
    x, c = torch.zeros(1, 64, 8), torch.zeros(1, 80, 8)
    h = torch.zeros(1, 64, 4)
    with pytest.raises(ValueError, match="PWGStream"):
        layers.WaveNetResidualBlock(dilation=2, use_causal_conv=True).lookahead_forward(x, c, None, 2, (None, h))
    small = layers.WaveNetResidualBlock(residual_channels=32, gate_channels=64, skip_channels=32)
    assert "channels" in small.lookahead_unsupported_reason()
    with pytest.raises(RuntimeError, match="channels"):
        small.lookahead_forward(torch.zeros(1, 32, 8), c, None, 1, (None, torch.zeros(1, 32, 2)))
    blk = layers.WaveNetResidualBlock(dilation=2)
    assert blk.lookahead_unsupported_reason(2, 7, 9) is None
    assert "negative" in blk.lookahead_unsupported_reason(2, 7, -1)
    blk.conv.precision = "bf16"
    with pytest.raises(RuntimeError, match="bf16"):
        blk.lookahead_forward(x, c, None, 2, (None, h))


# ---- latency and plan ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,latency", [({}, 3921), (SMALL, 66), (DEEP, 1075)])
def test_latency_from_the_geometry(cfg, latency):
    assert PWGLookaheadStream.latency_samples_of(models.ParallelWaveGANGenerator(**cfg)) == latency


def test_plan_of_the_small_config():
    """(kind, rate, delay, c_delay, state) per launch, by hand from the rules: conv_in is w = 2 frames late and keeps
    2 w frames; a stage of scale 4 takes D to 4 D + 4 and keeps 2 columns; the noise waits 52 columns; a layer of
    dilation d adds d, reads the conditioning sum(d so far) late, keeps 2 d columns and, from the second on, a skip
    line of d."""
    m = models.ParallelWaveGANGenerator(**SMALL)
    expected = [("conv_in", 1, 2, 0, [(80, 4)]), ("stage", 4, 12, 0, [(80, 2)]), ("stage", 16, 52, 0, [(80, 2)]),
                ("noise", 16, 52, 0, [(1, 52)]), ("first_conv", 16, 52, 0, []), ("cond_line", 16, 52, 0, [(80, 14)]),
                ("layer", 16, 53, 1, [(64, 2)]), ("layer", 16, 55, 3, [(64, 4), (64, 2)]),
                ("layer", 16, 59, 7, [(64, 8), (64, 4)]), ("layer", 16, 60, 8, [(64, 2), (64, 1)]),
                ("layer", 16, 62, 10, [(64, 4), (64, 2)]), ("layer", 16, 66, 14, [(64, 8), (64, 4)]),
                ("last_conv", 16, 66, 0, []), ("last_conv", 16, 66, 0, [])]
    plan = m.lookahead_plan()
    assert [(p.kind, p.rate, p.delay, p.c_delay, list(p.state)) for p in plan] == expected
    assert plan[0].module is m.upsample_net.conv_in and plan[6].module is m.conv_layers[0]
    assert plan[-1].module is m.last_conv_layers[3]
    floats = 80 * 4 + 2 * 80 * 2 + 52 + 80 * 14 + 64 * 2 * 14 + 64 * (14 - 1)
    shapes = pwg_lookahead_state_shapes(plan, 3)
    assert sum(torch.Size(s).numel() for s in shapes) == 3 * floats
    assert all(s[0] == 3 for s in shapes) and len(shapes) == 3 + 1 + 1 + 6 + 5


def test_state_of_v1():
    plan = models.ParallelWaveGANGenerator().lookahead_plan()
    assert len(plan) == 1 + 4 + 3 + 30 + 2
    assert [p.delay for p in plan[:5]] == [2, 12, 52, 212, 852]
    layer = [p for p in plan if p.kind == "layer"]
    assert [p.c_delay for p in layer][::10] == [1, 1024, 2047] and layer[-1].c_delay == 3069
    floats = sum(ch * cols for p in plan for ch, cols in p.state)
    # histories, skip lines (all layers but the first, d = 1), conditioning line, conv_in + 4 stages, noise line
    assert floats == 64 * 6138 + 64 * 3068 + 80 * 3069 + (80 * 4 + 4 * 80 * 2) + 852
    assert 3.3e6 < 4 * floats < 3.4e6  # bytes per half and stream


def test_plain_upsample_network_plan():
    m = models.ParallelWaveGANGenerator(layers=6, stacks=2, aux_context_window=0, upsample_net="UpsampleNetwork",
                                        upsample_params={"upsample_scales": [4, 4]})
    plan = m.lookahead_plan()
    assert [(p.kind, p.delay) for p in plan[:3]] == [("stage", 4), ("stage", 20), ("noise", 20)]
    assert plan[-1].delay == 20 + 14


# ---- the rules, emulated -------------------------------------------------------------------------------------------
class PWGLookaheadEmulation:
    """The delay rules of DESIGN.md s11.6 in float64 torch, independent of the package's plan: every layer in causal
    form over ``concat(history, chunk)``, the conditioning and the running skip sum through delay lines, zeros stored
    outside ``[D, D + T * rate)``.  ``sd``: reference-format state dict."""

    def __init__(self, sd, cfg):
        self.sd = {k: v.double() for k, v in sd.items()}
        self.layers, self.stacks = cfg["layers"], cfg["stacks"]
        self.scales = cfg["upsample_params"]["upsample_scales"]
        self.w = cfg["aux_context_window"]
        self.up = 1
        for s in self.scales:
            self.up *= s
        self.state, self.cols, self.latency = {}, {}, None

    def _line(self, name, new, length, seed=None):
        """concat(state, new), remembering its last ``length`` columns; the state starts as ``seed`` or zeros."""
        b, ch, _ = new.shape
        if name not in self.state:
            self.state[name] = torch.zeros(b, ch, length, dtype=torch.float64) if seed is None else seed
        cat = torch.cat([self.state[name], new], -1)
        self.state[name] = cat[..., cat.shape[-1] - length:]
        return cat

    def _mask(self, name, y, delay, rate, total):
        done = self.cols.get(name, 0)
        tau = torch.arange(done, done + y.shape[-1])
        self.cols[name] = done + y.shape[-1]
        valid = tau >= delay
        if total is not None:
            valid &= tau < delay + total * rate
        return torch.where(valid, y, torch.zeros((), dtype=torch.float64))

    def push(self, z, c, total=None):
        """z (B, 1, n * up), c (B, C, n) float64 -> (B, n * up): the stream's next columns, ``self.latency`` late."""
        sd, w, n = self.sd, self.w, c.shape[-1]
        # conv_in: history 2 w, seeded with the first frame; w frames late
        win = self._line("conv_in", c, 2 * w, seed=c[..., :1].expand(-1, -1, 2 * w))
        c = self._mask("conv_in", F.conv1d(win, torch_cpu.get_weight(sd, "upsample_net.conv_in")), w, 1, total)
        delay, rate = w, 1
        for i, s in enumerate(self.scales):
            # the causal stage: left padding 2 s over the stretched concat(last 2 columns, chunk)
            win = self._line(f"stage{i}", c, 2)
            xs = F.interpolate(win.unsqueeze(1), scale_factor=(1, s), mode="nearest")
            y = F.conv2d(xs, torch_cpu.get_weight(sd, f"upsample_net.upsample.up_layers.{2 * i + 1}")).squeeze(1)
            assert y.shape[-1] == c.shape[-1] * s
            delay, rate = delay * s + s, rate * s
            c = self._mask(f"stage{i}", y, delay, rate, total)
        d_c = delay
        z = self._line("noise", z, d_c)[..., :n * self.up]
        x = F.conv1d(z, torch_cpu.get_weight(sd, "first_conv"), torch_cpu.get_bias(sd, "first_conv"))
        x = self._mask("first_conv", x, d_c, rate, total)
        per_stack = self.layers // self.stacks
        reach = sum(2 ** (l % per_stack) for l in range(self.layers))
        c_cat = self._line("cond", c, reach)  # column reach + j of it is column j of the chunk
        skips = None
        for l in range(self.layers):
            p, d = f"conv_layers.{l}", 2 ** (l % per_stack)
            win = self._line(p + ":hist", x, 2 * d)
            h = F.conv1d(win, torch_cpu.get_weight(sd, p + ".conv"), torch_cpu.get_bias(sd, p + ".conv"), dilation=d)
            delay += d
            c_delay = delay - d_c
            a = F.conv1d(c_cat[..., reach - c_delay:reach - c_delay + x.shape[-1]], torch_cpu.get_weight(sd, p + ".conv1x1_aux"))
            zz = h + a
            g = torch.tanh(zz[:, :zz.shape[1] // 2]) * torch.sigmoid(zz[:, zz.shape[1] // 2:])
            s = F.conv1d(g, torch_cpu.get_weight(sd, p + ".conv1x1_skip"), torch_cpu.get_bias(sd, p + ".conv1x1_skip"))
            if skips is not None:
                s = s + self._line(p + ":skips", skips, d)[..., :x.shape[-1]]
            residual = win[..., d:d + x.shape[-1]]  # the middle tap
            x = (F.conv1d(g, torch_cpu.get_weight(sd, p + ".conv1x1_out"), torch_cpu.get_bias(sd, p + ".conv1x1_out"))
                 + residual) * math.sqrt(0.5)
            x = self._mask(p + ":x", x, delay, rate, total)
            skips = self._mask(p + ":s", s, delay, rate, total)
        skips = skips * math.sqrt(1.0 / self.layers)
        x = F.conv1d(F.relu(skips), torch_cpu.get_weight(sd, "last_conv_layers.1"), torch_cpu.get_bias(sd, "last_conv_layers.1"))
        x = self._mask("last1", x, delay, rate, total)
        y = F.conv1d(F.relu(x), torch_cpu.get_weight(sd, "last_conv_layers.3"), torch_cpu.get_bias(sd, "last_conv_layers.3"))
        self.latency = delay
        return self._mask("last3", y, delay, rate, total)[:, 0]


@pytest.mark.parametrize("frames", [1, 23])
def test_emulated_rules_equal_the_whole_utterance_oracle(frames):
    m = models.ParallelWaveGANGenerator(**SMALL)
    sd = synth_for(m, 31, 1.0)
    c = synth.synth_input("c", (2, 80, frames), seed=31).double()
    z = synth.synth_input("z", (2, 1, frames * 16), seed=31).double()
    ref = torch_cpu.pwg_generator({k: v.double() for k, v in sd.items()}, z, F.pad(c, (2, 2), mode="replicate"), **SMALL)[:, 0]
    rnd = random.Random(frames)
    pieces = []
    while sum(pieces) < frames:
        pieces.append(rnd.randint(1, min(5, frames - sum(pieces))))
    em, t, outs = PWGLookaheadEmulation(sd, SMALL), 0, []
    for n in pieces:
        outs.append(em.push(z[..., t * 16:(t + n) * 16], c[..., t:t + n]))
        t += n
    assert em.latency == PWGLookaheadStream.latency_samples_of(m) == 66
    for _ in range(-(-em.latency // em.up)):  # the flush: copies of the last frame, zero noise, the length known
        outs.append(em.push(torch.zeros(2, 1, 16, dtype=torch.float64), c[..., -1:], frames))
    y = torch.cat(outs, -1)
    front, body, back = y[:, :66], y[:, 66:66 + frames * 16], y[:, 66 + frames * 16:]
    assert max_abs(body, ref) < 1e-10
    assert float(front.abs().max()) == 0.0 and float(back.abs().max()) == 0.0  # exact zeros around the utterance


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_refusals_come_before_the_device_check():
    cfg = SMALL
    with pytest.raises(ValueError, match="PWGStream"):
        PWGLookaheadStream(models.ParallelWaveGANGenerator(**synth.PWG_CAUSAL))
    with pytest.raises(ValueError, match="MelGANGenerator is not supported"):
        PWGLookaheadStream(models.MelGANGenerator(channels=64, upsample_scales=[4, 2, 2], stacks=2))
    with pytest.raises(ValueError, match="HiFiGANGenerator.*LookaheadStream"):
        PWGLookaheadStream(models.HiFiGANGenerator(**synth.HIFIGAN_TINY))
    mel_up = models.ParallelWaveGANGenerator(
        layers=6, stacks=2, aux_context_window=0, upsample_net="MelGANGenerator",
        upsample_params=dict(upsample_scales=[4, 4], in_channels=80, out_channels=80, channels=64, stacks=1))
    with pytest.raises(ValueError, match="upsample_net='MelGANGenerator'"):
        PWGLookaheadStream(mel_up)
    with pytest.raises(ValueError, match="upsample_conditional_features"):
        PWGLookaheadStream(models.ParallelWaveGANGenerator(**dict(cfg, upsample_conditional_features=False)))
    linear = models.ParallelWaveGANGenerator(**cfg)
    linear.upsample_net.upsample.up_layers[0].mode = "linear"  # (the constructor builds only "nearest")
    with pytest.raises(ValueError, match="nearest"):
        PWGLookaheadStream(linear)
    with pytest.raises(ValueError, match="freq_axis_kernel_size"):
        PWGLookaheadStream(models.ParallelWaveGANGenerator(
            **dict(cfg, upsample_params={"upsample_scales": [4, 4], "freq_axis_kernel_size": 3})))
    with pytest.raises(ValueError, match=r"channels = 32 / 64 / 32"):  # the kernel's own reason (pwg_last_error)
        PWGLookaheadStream(models.ParallelWaveGANGenerator(**dict(cfg, residual_channels=32, gate_channels=64,
                                                                  skip_channels=32)))
    with pytest.raises(ValueError, match=r"in_channels / out_channels = 1 / 2"):
        PWGLookaheadStream(models.ParallelWaveGANGenerator(**dict(cfg, out_channels=2)))
    with pytest.raises(ValueError, match="batch"):
        PWGLookaheadStream(models.ParallelWaveGANGenerator(**cfg), batch=0)
    bf16 = models.ParallelWaveGANGenerator(**cfg)
    utils.set_inference_precision(bf16, "bf16")
    with pytest.raises(ValueError, match="bf16"):
        PWGLookaheadStream(bf16)
    # a supported non-causal model on the CPU: only the device is missing
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PWGLookaheadStream(models.ParallelWaveGANGenerator(**cfg))
    # the causal stream and the HiFi-GAN look-ahead stream keep refusing it
    with pytest.raises(ValueError, match="use_causal_conv"):
        utils.PWGStream(models.ParallelWaveGANGenerator(**cfg))
    with pytest.raises(ValueError, match="ParallelWaveGANGenerator"):
        utils.LookaheadStream(models.ParallelWaveGANGenerator(**cfg))
    assert PWGLookaheadStream.warmup_frames == 1


def test_causal_generator_and_networks_have_no_lookahead_plan():
    causal = models.ParallelWaveGANGenerator(**synth.PWG_CAUSAL)
    with pytest.raises(ValueError, match="PWGStream"):
        causal.lookahead_plan()
    with pytest.raises(ValueError, match="causal"):
        causal.upsample_net.lookahead_plan()
    with pytest.raises(ValueError, match="causal"):
        causal.upsample_net.upsample.lookahead_plan(80)
