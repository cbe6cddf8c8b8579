"""CPU: host logic of the look-ahead stream of the NON-causal (multi-band) MelGAN (utils.MelGANLookaheadStream, the
mirrored form of the streaming convolution) -- the mirror rule itself, emulated in float64 torch against
the whole-utterance oracle; the latencies, the delay plan, the settling and minimum lengths; what the kernel and the
stream refuse, and in which order.  Nothing here launches a kernel."""
import ctypes
import random

import pytest
import torch
import torch.nn.functional as F

from oracle import torch_cpu
from parallelwavegan_amd import _lib, layers, models, ops
from parallelwavegan_amd.layers.causal_conv import (LookaheadWalk, launch_is_mirrored, lookahead_state_shapes,
                                                    mirrored_delay, mirrored_desc, mirrored_in_window)
from parallelwavegan_amd.utils import LookaheadStream, MelGANLookaheadStream, PWGLookaheadStream, set_inference_precision
from tests.golden import synth
from tests.util import max_abs, synth_for

TINY = dict(synth.MELGAN_CAUSAL, use_causal_conv=False)  # channels 64, scales [4, 2, 2], 2 stacks
TINY_MB = dict(in_channels=80, out_channels=4, kernel_size=7, channels=32, upsample_scales=[3, 2], stack_kernel_size=3,
               stacks=3)  # an odd stride; dilations 1, 3, 9
V1 = dict()  # the constructor's defaults are melgan.v1: scales [8, 8, 2, 2], 3 stacks, 512 channels
MB_V2 = dict(out_channels=4, channels=384, upsample_scales=[8, 4, 2], stacks=4)      # multi_band_melgan.v2 (LJSpeech)
MB_V2_24K = dict(out_channels=4, channels=384, upsample_scales=[5, 5, 3], stacks=4)  # its 24 kHz variants, hop 300
PQMF_TAPS = 62


def _why():
    return _lib.lib().pwg_last_error().decode()


def _multi_band(cfg):
    g = models.MelGANGenerator(**cfg)
    if cfg.get("out_channels", 1) > 1:
        g.pqmf = layers.PQMF(subbands=cfg["out_channels"])
    return g


# ---- the rules, emulated -------------------------------------------------------------------------------------------
class MelGANEmulation:
    """The rules of DESIGN.md s11.8 in float64 torch, independent of the package's plan: every layer in causal form
    over ``concat(history, chunk)``; the history RAW (stored zeros, or the flush's dummy frames, outside the utterance);
    a reflect-padded layer maps every window column through the mirror at its input's valid window before it reads;
    the skip branch of a stack through a delay line; zeros stored outside ``[D, D + T * rate)``.  It also counts, per
    launch, the frames after which the launch has no edge in reach (``settle``) and the frames reflection needs
    (``min_frames``).  ``sd``: reference-format state dict."""

    def __init__(self, sd, cfg):
        self.sd = {k: v.double() for k, v in sd.items()}
        self.cfg = cfg
        self.state, self.cols = {}, {}
        self.latency = None
        self.settle, self.min_frames = 0, 1

    def _line(self, name, new, length):
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
        self.settle = max(self.settle, -(-delay // rate))
        return torch.where(valid, y, torch.zeros((), dtype=torch.float64))  # stored zeros, also where y is not finite

    def _mirrored(self, name, x, d_in, rate, total, dilation=1, slope=None, post=None):
        w, b = torch_cpu.get_weight(self.sd, name), torch_cpu.get_bias(self.sd, name)
        reach = (w.shape[-1] - 1) * dilation
        assert reach % 2 == 0
        p, n = reach // 2, x.shape[-1]
        done = self.cols.get(name, 0)  # input columns before this chunk (the layer has stride 1)
        cat = self._line(name + ":hist", x, reach)  # raw: window column t = -reach .. n - 1 at index t + reach
        in_lo = d_in - done
        in_hi = None if total is None else d_in + total * rate - done
        t = torch.arange(-reach, n)
        m = torch.where(t < in_lo, 2 * in_lo - t, t)
        if in_hi is not None:
            m = torch.where((t >= in_lo) & (t >= in_hi), 2 * (in_hi - 1) - t, m)
        live = (m >= -reach) & (m < n)
        win = torch.where(live, cat[..., (m + reach).clamp(0, reach + n - 1)], torch.zeros((), dtype=torch.float64))
        y = F.conv1d(win if slope is None else F.leaky_relu(win, slope), w, b, dilation=dilation)
        assert y.shape[-1] == n
        if post is not None:
            y = post(y)
        self.settle = max(self.settle, -(-(d_in + reach) // rate))  # the left edge has left the history
        self.min_frames = max(self.min_frames, p // rate + 1)       # frames * rate > p
        return self._mask(name, y, d_in + p, rate, total), d_in + p

    def _pointwise(self, name, x, d_in, rate, total, slope=None, addend=None):
        w, b = torch_cpu.get_weight(self.sd, name), torch_cpu.get_bias(self.sd, name)
        assert w.shape[-1] == 1
        y = F.conv1d(x if slope is None else F.leaky_relu(x, slope), w, b)
        if addend is not None:
            a, d_a = addend
            assert d_in >= d_a
            y = y + self._line(name + ":add", a, d_in - d_a)[..., :x.shape[-1]]
        return self._mask(name, y, d_in, rate, total), d_in

    def _up(self, name, x, d_in, rate_in, s, slope, total):
        w, b = torch_cpu.get_weight(self.sd, name), torch_cpu.get_bias(self.sd, name)
        d_out = d_in * s + s // 2 + s % 2
        win = self._line(name + ":hist", x, 1)
        n = x.shape[-1]
        y = F.conv_transpose1d(F.leaky_relu(win, slope), w, b, stride=s)[..., s:s + n * s]
        return self._mask(name, y, d_out, rate_in * s, total), d_out

    def push(self, c, total=None):
        """c: (B, C, n) float64 -> (B, out_channels, n * up): the next columns, still late by ``self.latency``."""
        cfg, slope = self.cfg, 0.2
        x, d = self._mirrored("melgan.1", c, 0, 1, total)
        rate, idx = 1, 2
        for s in cfg["upsample_scales"]:
            x, d = self._up(f"melgan.{idx + 1}", x, d, rate, s, slope, total)
            rate *= s
            idx += 2
            for j in range(cfg["stacks"]):
                pre = f"melgan.{idx}"
                skip = self._pointwise(pre + ".skip_layer", x, d, rate, total)
                t, dt = self._mirrored(pre + ".stack.2", x, d, rate, total, cfg["stack_kernel_size"] ** j, slope)
                x, d = self._pointwise(pre + ".stack.4", t, dt, rate, total, slope, addend=skip)
                idx += 1
        y, self.latency = self._mirrored(f"melgan.{idx + 2}", x, d, rate, total, 1, slope, post=torch.tanh)
        return y


def emulate(sd, cfg, c, pieces, flush_one_by_one=False):
    """Whole emulated utterance: ``c`` (B, C, T) in ``pieces``, then ``ceil(latency / up)`` DUMMY frames (random: their
    content must not matter) with the utterance's length known -> (the late stream (B, K, columns), the emulation)."""
    em, t, outs = MelGANEmulation(sd, cfg), 0, []
    total = c.shape[-1]
    for n in pieces:
        outs.append(em.push(c[..., t:t + n].double()))
        t += n
    assert t == total
    up = outs[0].shape[-1] // pieces[0]
    tail = -(-em.latency // up)
    gen = torch.Generator().manual_seed(5)
    dummy = 3.0 * torch.randn(c.shape[0], c.shape[1], tail, generator=gen, dtype=torch.float64)
    for lo, hi in ([(i, i + 1) for i in range(tail)] if flush_one_by_one else [(0, tail)]):
        outs.append(em.push(dummy[..., lo:hi], total))
    return torch.cat(outs, -1), em


def _pieces(kind, frames):
    if kind == "ones":
        return (1,) * frames
    if kind == "whole":
        return (frames,)
    rnd, pieces = random.Random(frames), []
    while sum(pieces) < frames:
        pieces.append(rnd.randint(1, min(5, frames - sum(pieces))))
    return tuple(pieces)


def _pqmf_synthesis64(x, subbands):
    """``torch_cpu.pqmf_synthesis`` on float64 columns: the oracle's own filters and steps, cast to double (the oracle
    itself computes in the filters' fp32, which cannot show 1e-10)."""
    _, hs = torch_cpu.pqmf_filters(subbands, PQMF_TAPS, 0.142, 9.0)
    up = F.conv_transpose1d(x, torch_cpu._updown(subbands).double() * subbands, stride=subbands)
    return F.conv1d(F.pad(up, (PQMF_TAPS // 2, PQMF_TAPS // 2)), hs.double())


def _pqmf_latency(k):
    return k * -(-(PQMF_TAPS // 2) // k)  # the K samples of a position leave once ceil(pad / K) more columns arrived


@pytest.mark.parametrize("kind,frames", [("ones", 9), ("random", 20), ("whole", 13), ("minimum", None)])
@pytest.mark.parametrize("cfg", [TINY, TINY_MB], ids=["tiny", "tiny_mb"])
def test_emulated_rules_equal_the_whole_utterance_oracle(cfg, kind, frames):
    g = _multi_band(cfg)
    sd = synth_for(models.MelGANGenerator(**cfg), 21, synth.MELGAN_G_SCALE)  # (without the PQMF's fixed filters)
    if kind == "minimum":  # both mirrors of the first layer (and of the widest stack) fall in one window
        frames, kind = MelGANLookaheadStream.min_frames_of(g), "whole"
        assert frames == 4
    c = synth.synth_input("c", (2, 80, frames), seed=21)
    ref = torch_cpu.melgan_generator({k: v.double() for k, v in sd.items()}, c.double(), **cfg)
    y, em = emulate(sd, cfg, c, _pieces(kind, frames), flush_one_by_one=(kind == "ones"))
    k, cols = ref.shape[1], ref.shape[-1]
    body, front, back = y[..., em.latency:em.latency + cols], y[..., :em.latency], y[..., em.latency + cols:]
    assert max_abs(body, ref) < 1e-10
    assert float(front.abs().max()) == 0.0 and float(back.abs().max()) == 0.0  # exact zeros around the utterance
    assert back.shape[-1] >= 0 and y.shape[-1] >= em.latency + cols
    latency = em.latency
    if k > 1:
        # the PQMF synthesis of the late stream is the late synthesis: the stored zeros are its zero padding
        wave, ref_wave = _pqmf_synthesis64(y, k)[:, 0], _pqmf_synthesis64(ref, k)[:, 0]
        assert max_abs(ref_wave.float(), torch_cpu.pqmf_synthesis(ref.float(), subbands=k)[:, 0]) < 1e-5
        assert max_abs(wave[:, em.latency * k:em.latency * k + cols * k], ref_wave) < 1e-10
        latency = em.latency * k + _pqmf_latency(k)
    # what the stream emits: frames * hop samples, latency_samples late
    assert cols * k == frames * g.upsample_factor * k
    assert MelGANLookaheadStream.latency_samples_of(g) == latency
    assert MelGANLookaheadStream.min_frames_of(g) == em.min_frames
    hop = g.upsample_factor * k
    assert MelGANLookaheadStream.settle_frames_of(g) == max(em.settle, -(-latency // hop))


# ---- latencies, the plan, settling -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,columns,latency,settle,min_frames", [
    (TINY, 90, 90, 6, 4), (TINY_MB, 65, 65 * 4 + 32, 13, 4), (V1, 1425, 1425, 7, 4), (MB_V2, 672, 672 * 4 + 32, 12, 4), (MB_V2_24K, 1044, 1044 * 4 + 32, 17, 6)],
    ids=["tiny", "tiny_mb", "melgan.v1", "multi_band_melgan.v2", "multi_band_melgan.v2 [5, 5, 3]"])
def test_latency_settling_and_minimum_from_the_geometry(cfg, columns, latency, settle, min_frames):
    g = _multi_band(cfg)
    assert g.lookahead_plan()[-1].delay == columns
    assert MelGANLookaheadStream.latency_samples_of(g) == latency
    assert MelGANLookaheadStream.settle_frames_of(g) == settle
    assert MelGANLookaheadStream.min_frames_of(g) == min_frames
    # the emulation's own count, on one whole push of synthetic weights (tiny ones only: the big ones are GPU-sized)
    if cfg in (TINY, TINY_MB):
        sd = synth_for(models.MelGANGenerator(**cfg), 3, 1.0)
        _, em = emulate(sd, cfg, synth.synth_input("c", (1, 80, 5), seed=3), (5,))
        assert (em.latency, em.min_frames) == (columns, min_frames)


def test_delay_plan_of_the_tiny_config():
    """(rate, delay, delay1, delay2) per launch, by hand: a reflect-padded Conv1d adds its padding, a ConvTranspose1d
    gives D * s + s//2 + s%2, a stack is skip 1 x 1 (at D), dilated conv (D + d), 1 x 1 (D + d, skip d older)."""
    def stack(rate, d0, d):
        return [(rate, d0, 0, 0), (rate, d0 + d, 0, 0), (rate, d0 + d, d, 0)]

    expected = [(1, 3, 0, 0)]
    expected += [(4, 14, 0, 0)] + stack(4, 14, 1) + stack(4, 15, 3)
    expected += [(8, 37, 0, 0)] + stack(8, 37, 1) + stack(8, 38, 3)
    expected += [(16, 83, 0, 0)] + stack(16, 83, 1) + stack(16, 84, 3)
    expected += [(16, 90, 0, 0)]
    g = models.MelGANGenerator(**TINY)
    plan = g.lookahead_plan()
    assert [tuple(launch[1:]) for launch in plan] == expected
    assert plan[0].conv is g.melgan[1] and plan[1].conv is g.melgan[3] and plan[-1].conv is g.melgan[-2]
    assert plan[2].conv is g.melgan[4].skip_layer and plan[3].conv is g.melgan[4].stack[2]
    # the reflect-padded launches are the mirrored ones: first, last, each stack's dilated convolution
    assert [launch_is_mirrored(launch) for launch in plan] == [True] + ([False] + [False, True, False] * 2) * 3 + [True]
    shapes = lookahead_state_shapes(plan, 2)
    assert shapes[:5] == [(2, 80, 6), (2, 64, 1), (2, 32, 2), (2, 32, 1), (2, 32, 6)]  # hist, hist, hist, skip line, hist
    for launch in plan:
        if launch_is_mirrored(launch):
            assert ops.conv1d_stream_mirrored_supported(mirrored_desc(launch.conv, 2, 8)), _why()


def test_every_launch_of_the_recipes_fits_the_kernels():
    from parallelwavegan_amd.layers.causal_conv import launch_desc

    for cfg in (V1, MB_V2, MB_V2_24K):
        for launch in models.MelGANGenerator(**cfg).lookahead_plan():
            for batch, n in ((1, 1), (16, 8)):
                d = launch_desc(launch, batch, n)
                ok = ops.conv1d_stream_mirrored_supported(d) if launch_is_mirrored(launch) else \
                    ops.conv1d_stream_delayed_supported(d, launch.delay1, launch.delay2)
                assert ok, (launch, _why())


def test_input_window_of_a_mirrored_launch():
    g = models.MelGANGenerator(**TINY)
    plan = g.lookahead_plan()
    first, dilated = plan[0], plan[6]  # (rate 1, delay 3, pad 3), (rate 4, delay 18, pad 3)
    assert mirrored_in_window(first, 0) == (0, None) and mirrored_in_window(first, 5) == (-5, None)
    assert mirrored_in_window(first, 5, 5) == (-5, 0)
    assert mirrored_in_window(dilated, 2) == (15 - 8, None) and mirrored_in_window(dilated, 9, 9) == (15 - 36, 15)
    lo, hi = mirrored_in_window(first)  # steady state: no edge in reach of any window
    assert lo <= -144 and hi is None


# ---- the kernel's query --------------------------------------------------------------------------------------------
def test_mirrored_supported_answers_without_a_device():
    def desc(k=7, d=1, **kw):
        kw.setdefault("pad_left", (k - 1) * d)
        kw.setdefault("pad_mode", "reflect")
        return ops.make_conv_desc(2, 24, 40, 9, kw.pop("t_out", 9), k, dilation=d, **kw)

    for k, d in ((7, 1), (3, 9), (3, 27), (3, 72), (1, 1)):
        assert ops.conv1d_stream_mirrored_supported(desc(k, d)), (k, d, _why())
    assert not ops.conv1d_stream_mirrored_supported(desc(pad_mode="zero")) and "pad_mode" in _why()
    assert not ops.conv1d_stream_mirrored_supported(desc(pad_mode="replicate")) and "pad_mode" in _why()
    dt = ops.make_conv_desc(2, 24, 12, 9, 36, 8, stride=4, pad_left=4, transposed=True)
    assert not ops.conv1d_stream_mirrored_supported(dt) and "transposed" in _why()
    strided = ops.make_conv_desc(2, 24, 40, 9, 9, 7, stride=2, pad_left=6, pad_mode="reflect")
    assert not ops.conv1d_stream_mirrored_supported(strided) and "stride" in _why()
    assert not ops.conv1d_stream_mirrored_supported(desc(4, 1)) and "odd" in _why()       # history 3
    assert not ops.conv1d_stream_mirrored_supported(desc(3, 73)) and "LDS" in _why()      # history 146 > 144
    assert not ops.conv1d_stream_mirrored_supported(desc(groups=4, pad_left=6)) and "groups" in _why()
    # a symmetric (whole-utterance) descriptor is not the layer's causal form
    assert not ops.conv1d_stream_mirrored_supported(desc(pad_left=3)) and "causal" in _why()
    # the delayed entry points keep refusing what the mirrored one takes
    assert not ops.conv1d_stream_delayed_supported(desc()) and "pad_mode" in _why()
    assert not ops.conv1d_stream_bf16_delayed_supported(desc()) and "pad_mode" in _why()


def test_mirrored_entry_points_are_exported_under_the_same_abi():
    assert _lib.ABI_VERSION == _lib.lib().pwg_abi_version() == 15
    for name in ("pwg_conv1d_stream_mirrored_supported", "pwg_conv1d_stream_mirrored_forward"):
        assert name in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)


def test_mirrored_forward_refuses_cpu_tensors():
    d = ops.make_conv_desc(1, 4, 4, 8, 8, 3, pad_left=2, pad_mode="reflect")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.conv1d_stream_mirrored_forward(d, torch.zeros(1, 4, 8), None, torch.zeros(1, 4, 2), torch.zeros(3 * 16 * 128))


def test_mirrored_delay_refuses_layers_without_the_form():
    assert mirrored_delay(layers.Conv1d(8, 8, 3, dilation=9, padding=9, pad_mode="reflect"), 5) == 14
    with pytest.raises(ValueError, match="reflect"):
        mirrored_delay(layers.Conv1d(8, 8, 3, padding=1), 0)
    with pytest.raises(ValueError, match="even kernel"):
        mirrored_delay(layers.Conv1d(8, 8, 4, padding=(1, 2), pad_mode="reflect"), 0)
    with pytest.raises(ValueError, match="symmetric"):
        mirrored_delay(layers.Conv1d(8, 8, 3, padding=(2, 0), pad_mode="reflect"), 0)


# ---- what the stream refuses, and in which order ---------------------------------------------------------------------
def test_stream_refuses_models_it_cannot_stream_before_any_device_check():
    # (all of these models live on the CPU: a refusal that names the model comes before "no CPU fallback")
    with pytest.raises(ValueError, match="HiFiGANGenerator is not supported"):
        MelGANLookaheadStream(models.HiFiGANGenerator(**synth.HIFIGAN_TINY))
    with pytest.raises(ValueError, match="CausalStream"):
        MelGANLookaheadStream(models.MelGANGenerator(**synth.MELGAN_CAUSAL))
    with pytest.raises(ValueError, match="ReflectionPad1d"):
        MelGANLookaheadStream(models.MelGANGenerator(**dict(TINY, pad="ReplicationPad1d")))
    with pytest.raises(ValueError, match="ReflectionPad1d"):
        MelGANLookaheadStream(models.MelGANGenerator(**dict(TINY, pad="ConstantPad1d", pad_params={"value": 0.0})))
    # a layer the kernel turns down: (k - 1) * d = 2 * 81 = 162 columns of history
    with pytest.raises(ValueError, match="LDS"):
        MelGANLookaheadStream(models.MelGANGenerator(**dict(TINY, stacks=5)))
    with pytest.raises(ValueError, match="PQMF attached"):
        MelGANLookaheadStream(models.MelGANGenerator(**TINY_MB))
    g = _multi_band(TINY_MB)
    g.pqmf = layers.PQMF(subbands=3)
    with pytest.raises(ValueError, match="as many sub-bands"):
        MelGANLookaheadStream(g)
    g = models.MelGANGenerator(**TINY)
    with pytest.raises(ValueError, match="bf16.*does not exist"):
        MelGANLookaheadStream(g, precision="bf16")
    with pytest.raises(ValueError, match="precision must be"):
        MelGANLookaheadStream(g, precision="fp16")
    with pytest.raises(ValueError, match="batch"):
        MelGANLookaheadStream(g, batch=0)
    # order: a causal bf16-mode model is told about CausalStream, a non-causal one about its precision
    causal = models.MelGANGenerator(**synth.MELGAN_CAUSAL)
    set_inference_precision(causal, "bf16")
    with pytest.raises(ValueError, match="CausalStream"):
        MelGANLookaheadStream(causal)
    set_inference_precision(g, "bf16")
    with pytest.raises(ValueError, match="bf16 inference precision"):
        MelGANLookaheadStream(g)


def test_stream_on_a_cpu_model_has_no_fallback():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MelGANLookaheadStream(models.MelGANGenerator(**TINY))


def test_causal_and_other_paddings_have_no_lookahead_plan():
    with pytest.raises(ValueError, match="CausalStream"):
        models.MelGANGenerator(**synth.MELGAN_CAUSAL).lookahead_plan()
    with pytest.raises(ValueError, match="ReflectionPad1d"):
        models.MelGANGenerator(**dict(TINY, pad="ReplicationPad1d")).lookahead_plan()
    with pytest.raises(ValueError, match="CausalStream"):
        layers.ResidualStack(channels=8, use_causal_conv=True).lookahead_plan(0, 1)


def test_the_other_lookahead_streams_keep_refusing_a_melgan():
    g = models.MelGANGenerator(**TINY)
    with pytest.raises(ValueError, match="MelGANGenerator.*MelGANLookaheadStream"):
        LookaheadStream(g)
    with pytest.raises(ValueError, match="MelGANGenerator is not supported"):
        PWGLookaheadStream(g)


def test_a_bf16_walk_refuses_a_mirrored_launch():
    g = models.MelGANGenerator(**TINY)
    plan = g.lookahead_plan()
    walk = LookaheadWalk(plan, None, [None] * len(lookahead_state_shapes(plan, 1)), 0, None, precision="bf16")
    with pytest.raises(RuntimeError, match="no bf16 form"):
        walk.run(plan[0].conv, torch.zeros(1, 80, 4))
