"""GPU: the look-ahead stream of the NON-causal HiFi-GAN with bf16 operands (the delayed form of
csrc/conv1d_stream_bf16.hip, ``LookaheadStream(model, precision="bf16")``).

Layers: the delayed bf16 launch against the plain bf16 launch bit for bit (the delay lines and the valid window change
nothing inside the window), its state against the fp32 delayed launch's bit for bit (state is raw fp32 in either
precision), and against float64 of the same bf16-rounded operands at the project's per-layer bar (RTOL of
tests/test_conv_bf16_gpu.py; with a pre-activation the ACTIVATED input is what is rounded before the call).
Generator: any partition of the same frames gives the same bits, and the error against the fp32 oracle is the CPU
emulation's error (FACTOR of tests/test_hifigan_bf16_gpu.py)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import torch_cpu
from parallelwavegan_amd import layers, models, ops
from parallelwavegan_amd.layers.causal_conv import lookahead_desc, lookahead_history_columns
from parallelwavegan_amd.layers.conv import each_conv
from parallelwavegan_amd.utils import LookaheadStream
from tests.bf16_emulation import bf16_operands, rms
from tests.golden import synth
from tests.test_conv_bf16_gpu import RTOL
from tests.test_hifigan_bf16_gpu import FACTOR
from tests.test_stream_lookahead_gpu import (CHUNKS, FUSED, PIECES, TINY_FRAMES, TINY_LATENCY, TINY_UP, _stream, _tiny_case,
                                             _tiny_model)
from tests.util import max_abs, poison_lds, synth_for

pytestmark = pytest.mark.gpu

BF16_DELAYED, FP32_DELAYED = "conv1d_stream_bf16_delayed_kernel", "conv1d_stream_delayed_kernel"
OTHER_CONVS = ("conv1d_stream_kernel", FP32_DELAYED, "conv1d_mfma_dma_kernel", "conv1d_bf16_mfma_kernel")
# the two layers of tests/test_stream_lookahead_gpu.py; 160 input channels: five chunks in two staged blocks, 24 rows: no
# multiple of 16; 64 -> 5 x 2: 10 image rows, two chunks
LAYERS = {
    "conv": lambda: layers.Conv1d(24, 40, 5, dilation=3, padding=6),
    "up": lambda: layers.ConvTranspose1d(24, 12, 8, 4, padding=2),
    "conv160": lambda: layers.Conv1d(160, 24, 3, padding=1),
    "up64": lambda: layers.ConvTranspose1d(64, 5, 4, 2, padding=1),
}
KINDS = list(LAYERS)


def _layer(kind, device):
    """-> (layer on the device, output columns per input column)"""
    torch.manual_seed(9)
    cv = LAYERS[kind]()
    return cv.to(device), (cv.stride if cv.transposed else 1)


def _rand(gen, *shape):
    return torch.randn(*shape, generator=gen)


def _nan(device, *shape):
    return torch.full(shape, float("nan"), device=device)


def _bf16r(t):
    return t.to(torch.bfloat16).to(torch.float32)


# ---- 1. no delay, full window: the plain bf16 launch ---------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_no_delay_full_window_equals_the_plain_bf16_launch(kind, device):
    cv, s = _layer(kind, device)
    gen = torch.Generator().manual_seed(31)
    c_in, c_out, h_cols = cv.in_channels, cv.out_channels, lookahead_history_columns(cv)
    bias, w = cv.bias.detach(), cv.packed_weight_bf16()
    for n in CHUNKS:
        x, hist = _rand(gen, 2, c_in, n).to(device), _rand(gen, 2, c_in, h_cols).to(device)
        a1, a2 = (_rand(gen, 2, c_out, n * s).to(device) for _ in range(2))
        desc = lookahead_desc(cv, 2, n, **FUSED)
        for hist_in in (hist, None):  # (None: start of stream)
            h0, h1 = _nan(device, 2, c_in, h_cols), _nan(device, 2, c_in, h_cols)
            y0, y1 = _nan(device, 2, c_out, n * s), _nan(device, 2, c_out, n * s)
            ops.conv1d_stream_forward_bf16(desc, x, hist_in, h0, w, bias, a1, a2, out=y0)
            ops.conv1d_stream_delayed_forward_bf16(desc, x, hist_in, h1, w, bias, a1, (None, None), 0, a2, (None, None), 0,
                                                   valid=(0, n * s), out=y1)
            assert torch.isfinite(y0).all()
            assert torch.equal(y0, y1) and torch.equal(h0, h1), (kind, n)


# ---- 2. delays over pieces shorter than them -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_delayed_addends_equal_host_delayed_addends_and_the_fp32_state(kind, device):
    cv, s = _layer(kind, device)
    gen = torch.Generator().manual_seed(32)
    total, d1, d2 = sum(PIECES), 7, 30
    c_in, c_out, h_cols = cv.in_channels, cv.out_channels, lookahead_history_columns(cv)
    bias, w, w32 = cv.bias.detach(), cv.packed_weight_bf16(), cv.packed_weight()
    x = _rand(gen, 2, c_in, total).to(device)
    a1, a2 = (_rand(gen, 2, c_out, total * s).to(device) for _ in range(2))
    # delayed on the host: `delay` zero columns in front
    a1_late = torch.cat([torch.zeros(2, c_out, d1, device=device), a1], -1)
    a2_late = torch.cat([torch.zeros(2, c_out, d2, device=device), a2], -1)
    # [plain bf16, delayed bf16, delayed fp32][ping-pong]
    hist = [[_nan(device, 2, c_in, h_cols) for _ in range(2)] for _ in range(3)]
    line1, line2 = ([[_nan(device, 2, c_out, d) for _ in range(2)] for _ in range(2)] for d in (d1, d2))  # [bf16, fp32]
    t, cur = 0, None
    for n in PIECES:
        nxt = 0 if cur is None else 1 - cur
        pick = lambda bufs: (None if cur is None else bufs[cur], bufs[nxt])  # noqa: E731
        xs = x[..., t:t + n].contiguous()
        lo, hi = t * s, (t + n) * s
        p1, p2 = a1[..., lo:hi].contiguous(), a2[..., lo:hi].contiguous()
        desc = lookahead_desc(cv, 2, n, **FUSED)
        y_ref = ops.conv1d_stream_forward_bf16(desc, xs, *pick(hist[0]), w, bias, a1_late[..., lo:hi].contiguous(),
                                               a2_late[..., lo:hi].contiguous())
        y = ops.conv1d_stream_delayed_forward_bf16(desc, xs, *pick(hist[1]), w, bias, p1, pick(line1[0]), d1, p2,
                                                   pick(line2[0]), d2)
        ops.conv1d_stream_delayed_forward(desc, xs, *pick(hist[2]), w32, bias, p1, pick(line1[1]), d1, p2, pick(line2[1]), d2)
        assert torch.isfinite(y_ref).all()
        assert torch.equal(y, y_ref), (kind, t, n)
        # state: that of the fp32 delayed launch, bit for bit
        assert torch.equal(hist[1][nxt], hist[2][nxt]) and torch.equal(hist[1][nxt], hist[0][nxt])
        assert torch.equal(line1[0][nxt], line1[1][nxt]) and torch.equal(line2[0][nxt], line2[1][nxt])
        # the delay lines hold the last `delay` columns of concat(zeros, addend so far)
        assert torch.equal(line1[0][nxt], a1_late[..., hi:hi + d1]) and torch.equal(line2[0][nxt], a2_late[..., hi:hi + d2])
        cur, t = nxt, t + n


# ---- 3. the valid window -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_valid_window_stores_exact_zeros_outside(kind, poison, device):
    cv, s = _layer(kind, device)
    gen = torch.Generator().manual_seed(33)
    c_in, c_out, h_cols = cv.in_channels, cv.out_channels, lookahead_history_columns(cv)
    bias, w = cv.bias.detach(), cv.packed_weight_bf16()
    for n in CHUNKS:
        t_out = n * s
        x, hist = _rand(gen, 2, c_in, n).to(device), _rand(gen, 2, c_in, h_cols).to(device)
        a1, l1 = _rand(gen, 2, c_out, t_out).to(device), _rand(gen, 2, c_out, 7).to(device)
        desc = lookahead_desc(cv, 2, n, post_act="tanh", **FUSED)

        def run(valid):
            y = _nan(device, 2, c_out, t_out)
            ops.conv1d_stream_delayed_forward_bf16(desc, x, hist, _nan(device, 2, c_in, h_cols), w, bias, a1,
                                                   (l1, _nan(device, 2, c_out, 7)), 7, valid=valid, out=y)
            return y

        full = run(None)
        if poison:
            with poison_lds():
                y = run((3, t_out - 2))
        else:
            y = run((3, t_out - 2))
        assert torch.isfinite(full).all()
        assert torch.equal(y[..., 3:t_out - 2], full[..., 3:t_out - 2]), (kind, n)
        outside = torch.cat([y[..., :3], y[..., max(3, t_out - 2):]], -1)
        assert outside.numel() and torch.equal(outside, torch.zeros_like(outside)), (kind, n)


# ---- 4. against float64 of the same rounded operands ---------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_delayed_bf16_layer_matches_float64_of_rounded_operands(kind, device):
    """The layer in causal form from a zero start, both addends through delay lines of 7 and 30 columns, /3 and tanh,
    zeros outside the window [5, total - 4) of the stream -- over PIECES, against float64 of the bf16-rounded weights and
    the bf16-rounded ACTIVATED input."""
    cv, s = _layer(kind, device)
    g = torch.Generator().manual_seed(34)
    total, d1, d2 = sum(PIECES), 7, 30
    c_in, c_out, h_cols = cv.in_channels, cv.out_channels, lookahead_history_columns(cv)
    x = _bf16r(_rand(g, 2, c_in, total))
    w = _bf16r(cv.weight.detach().cpu())
    with torch.no_grad():
        cv.weight.copy_(w)
    b = cv.bias.detach().cpu()
    a1, a2 = _rand(g, 2, c_out, total * s), _rand(g, 2, c_out, total * s)
    xa = _bf16r(F.leaky_relu(x, FUSED["pre_slope"])).double()
    if cv.transposed:
        conv = F.conv_transpose1d(F.pad(xa, (1, 0)), w.double(), b.double(), stride=s)[:, :, s:-s]
    else:
        conv = torch_cpu.causal_conv1d(xa, w.double(), b.double(), cv.dilation)
    late = lambda a, d: torch.cat([torch.zeros(2, c_out, d), a], -1)[..., :total * s].double()  # noqa: E731
    ref = torch.tanh((conv + late(a1, d1) + late(a2, d2)) / FUSED["out_div"])
    lo_g, hi_g = 5, total * s - 4
    ref[..., :lo_g] = 0.0
    ref[..., hi_g:] = 0.0

    bias, image = cv.bias.detach(), cv.packed_weight_bf16()
    hist = [_nan(device, 2, c_in, h_cols) for _ in range(2)]
    line1, line2 = ([_nan(device, 2, c_out, d) for _ in range(2)] for d in (d1, d2))
    outs, t, cur = [], 0, None
    for n in PIECES:
        nxt = 0 if cur is None else 1 - cur
        pick = lambda bufs: (None if cur is None else bufs[cur], bufs[nxt])  # noqa: E731
        t_out, before = n * s, t * s
        valid = (min(max(lo_g - before, 0), t_out), min(max(hi_g - before, 0), t_out))
        desc = lookahead_desc(cv, 2, n, post_act="tanh", **FUSED)
        outs.append(ops.conv1d_stream_delayed_forward_bf16(
            desc, x[..., t:t + n].contiguous().to(device), *pick(hist), image, bias,
            a1[..., before:before + t_out].contiguous().to(device), pick(line1), d1,
            a2[..., before:before + t_out].contiguous().to(device), pick(line2), d2, valid))
        cur, t = nxt, t + n
    y = torch.cat(outs, -1).cpu().double()
    assert y.shape == ref.shape and torch.isfinite(y).all()
    assert torch.equal(y[..., :lo_g], torch.zeros_like(y[..., :lo_g])) and torch.equal(y[..., hi_g:], torch.zeros_like(y[..., hi_g:]))
    err = (y - ref).abs().max().item() / (ref.abs().max().item() + 1e-12)
    print(f"{kind}: delayed bf16 launch vs float64 of the rounded operands, rel-to-max error {err:.3e} (bar {RTOL:.1e})")
    assert err <= RTOL


# ---- 5. the pointer rules ------------------------------------------------------------------------------------------
def test_delay_line_buffers_must_be_distinct_and_present(device):
    cv, _ = _layer("conv", device)
    desc = lookahead_desc(cv, 1, 4)
    x, add = torch.zeros(1, 24, 4, device=device), torch.zeros(1, 40, 4, device=device)
    hist, line = torch.zeros(1, 24, 12, device=device), torch.zeros(1, 40, 7, device=device)
    with pytest.raises(RuntimeError, match="distinct"):
        ops.conv1d_stream_delayed_forward_bf16(desc, x, None, hist, cv.packed_weight_bf16(), None, add, (line, line), 7)
    with pytest.raises(RuntimeError, match="hist_out"):
        ops.conv1d_stream_delayed_forward_bf16(desc, x, None, hist, cv.packed_weight_bf16(), None, add, (None, None), 7)
    with pytest.raises(RuntimeError, match="distinct"):
        ops.conv1d_stream_delayed_forward_bf16(desc, x, hist, hist, cv.packed_weight_bf16())


# ---- 6. the streamed generator: partitions, bit for bit ------------------------------------------------------------
PARTITIONS = ((1,) * TINY_FRAMES, (3, 1, 7, 2, 5, 5))


def _bf16(model, c, pieces, **kw):
    kw.setdefault("use_graph", False)
    return _stream(model, c, pieces, precision="bf16", **kw)  # (checks the emission length after every push and flush)


def _check_tiny_partitions(device):
    model, c = _tiny_model(device), _tiny_case()[2].to(device)
    s = LookaheadStream(model, batch=2, use_graph=False, precision="bf16")
    assert s.precision == "bf16" and (s.latency_samples, s.latency_frames, s.up) == (TINY_LATENCY, 8, TINY_UP)
    whole = _stream(model, c, (TINY_FRAMES,), stream=s)
    assert torch.isfinite(whole).all() and whole.abs().max() > 1e-3
    for pieces in PARTITIONS:
        y = _bf16(model, c, pieces)
        assert torch.equal(y, whole), (pieces, max_abs(y, whole))
    # two lock-step streams equal two single ones
    for b in range(2):
        assert torch.equal(_bf16(model, c[b:b + 1], PARTITIONS[1])[0], whole[b])


def test_tiny_partitions_are_bit_identical(device):
    _check_tiny_partitions(device)


def test_tiny_partitions_are_bit_identical_with_poisoned_lds(device):
    with poison_lds():
        _check_tiny_partitions(device)


def test_emission_lengths_are_those_of_the_fp32_stream(device):
    model, c = _tiny_model(device), _tiny_case()[2].to(device)
    feats = c.transpose(1, 2).contiguous()
    a, b = LookaheadStream(model, batch=2, use_graph=False, precision="bf16"), LookaheadStream(model, batch=2, use_graph=False)
    assert a.state_bytes == b.state_bytes and [t.shape for t in a._halves[0]] == [t.shape for t in b._halves[0]]
    t = 0
    for n in PARTITIONS[1]:
        ya, yb = a.push(feats[:, t:t + n]), b.push(feats[:, t:t + n])
        t += n
        assert ya.shape == yb.shape and (a.frames_in, a.samples_out) == (b.frames_in, b.samples_out)
    # state fed by the features alone (the input convolution's history) is bit-identical: raw fp32 in either precision
    assert torch.equal(a._halves[a._cur][0], b._halves[b._cur][0])
    assert a.flush().shape == b.flush().shape and a.samples_out == b.samples_out == TINY_FRAMES * TINY_UP


@pytest.mark.parametrize("frames", [1, 2])
def test_utterance_shorter_than_the_latency(frames, device):
    model, c = _tiny_model(device), _tiny_case()[2][..., :frames].contiguous().to(device)
    y = _bf16(model, c, (1,) * frames)  # (every push returns empty: checked in _stream)
    assert y.shape == (2, frames * TINY_UP) and torch.isfinite(y).all()
    if frames == 2:
        assert torch.equal(_bf16(model, c, (2,)), y)
    assert y.abs().max() > 1e-3


def test_without_additional_convs(device):
    model, c = _tiny_model(device, False), _tiny_case(False)[2].to(device)
    whole = _bf16(model, c, (TINY_FRAMES,))
    assert torch.isfinite(whole).all() and whole.abs().max() > 1e-3
    for pieces in PARTITIONS:
        assert torch.equal(_bf16(model, c, pieces), whole), pieces


# ---- 7. whole generator, statistical -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_and_emulation(seed, g_scale, name, frames, c_seed):
    """(state dict, c = synth_input(name, (2, 80, frames), c_seed), fp32 oracle, the oracle with every convolution's operands rounded to bf16) on
    the CPU, computed once and never modified."""
    cfg = synth.HIFIGAN_TINY
    model = models.HiFiGANGenerator(**cfg)
    sd = synth_for(model, seed, g_scale)
    c = synth.synth_input(name, (2, 80, frames), seed=c_seed)
    with torch.no_grad():
        ref = torch_cpu.hifigan_generator(sd, c, **cfg)
        with bf16_operands() as stats:
            emu = torch_cpu.hifigan_generator(sd, c, **cfg)
    assert stats["untouched"] == 0 and stats["rounded"] == len(list(each_conv(model)))
    e_emu = rms(emu - ref)
    assert e_emu > 0
    return sd, c, ref[:, 0], e_emu


def _within_the_bar(y, ref, e_emu, what):
    assert y.shape == ref.shape and torch.isfinite(y).all()  # (no sample is left out)
    e_gpu = rms(y.cpu() - ref)
    print(f"{what}: rms(stream_bf16 - oracle) {e_gpu:.3e}, rms(emulation - oracle) {e_emu:.3e}, ratio {e_gpu / e_emu:.3f}, "
          f"rms(signal) {rms(ref):.3e}")
    assert e_gpu <= FACTOR * e_emu


def test_bf16_stream_error_is_the_emulations_error(device):
    """rms(stream_bf16 - oracle_fp32) <= FACTOR * rms(emulation - oracle_fp32); the emulation is the CPU oracle with
    every convolution's operands rounded (no predicate), as in the stream.  No sample is left out."""
    sd, c, ref, e_emu = _oracle_and_emulation(21, 1.0, "c", 36, 36)
    model = models.HiFiGANGenerator(**synth.HIFIGAN_TINY)
    model.load_state_dict(sd)
    model = model.to(device).eval()
    _within_the_bar(_bf16(model, c.to(device), (9, 8, 8, 1, 10)), ref, e_emu, "tiny, 36 frames")


# ---- 8. the mode is really on, and the default is untouched --------------------------------------------------------
def test_bf16_stream_is_really_on_and_default_is_untouched(device):
    model, never = _tiny_model(device), _tiny_model(device)
    n_convs = len(list(each_conv(model)))
    c = synth.synth_input("c24", (2, 80, 24), seed=22).to(device)
    feats = c.transpose(1, 2).contiguous()
    with torch.no_grad():
        whole_never = never(c)
    y32_never = _stream(never, c, (8, 8, 8), use_graph=False)

    s = LookaheadStream(model, batch=2, use_graph=False, precision="bf16")
    assert s.precision == "bf16"
    first = s.push(feats[:, :8])  # (start of stream; the weight images are built here, outside the profiled push)
    with ops.profile() as prof:
        second = s.push(feats[:, 8:16])
    assert prof.results[BF16_DELAYED]["launches"] == n_convs, prof.results
    assert not any(k in prof.results for k in OTHER_CONVS), prof.results
    y16 = torch.cat([first, second, s.push(feats[:, 16:]), s.flush()], -1)
    assert torch.isfinite(y16).all() and y16.shape == y32_never.shape and not torch.equal(y16, y32_never)
    assert torch.equal(_bf16(model, c, (8, 8, 8)), y16)  # deterministic

    # the default stream built afterwards on the same model: the fp32 kernel, bit-identical to a model that never saw bf16
    assert all(cv.precision == "fp32" for cv in each_conv(model))
    s32 = LookaheadStream(model, batch=2, use_graph=False)
    assert s32.precision == "fp32" and LookaheadStream(model, batch=2, precision="fp32").precision == "fp32"
    s32.push(feats[:, :8])
    with ops.profile() as prof:
        s32.push(feats[:, 8:16])
    assert prof.results[FP32_DELAYED]["launches"] == n_convs and BF16_DELAYED not in prof.results, prof.results
    assert torch.equal(_stream(model, c, (8, 8, 8), use_graph=False), y32_never)
    assert torch.equal(_stream(model, c, (8, 8, 8), use_graph=False, precision="fp32"), y32_never)
    with torch.no_grad():
        assert torch.equal(model(c), whole_never)
    assert all(cv.precision == "fp32" for cv in each_conv(model))


# ---- 9. graph mode -------------------------------------------------------------------------------------------------
def test_graph_mode(device):
    model = _tiny_model(device)
    c = synth.synth_input("c24", (2, 80, 24), seed=22).to(device)
    c2 = synth.synth_input("c24b", (2, 80, 24), seed=23).to(device)
    eager = _bf16(model, c, (4,) * 6)
    s = LookaheadStream(model, batch=2, use_graph=True, precision="bf16")
    feats = c.transpose(1, 2).contiguous()
    outs = []
    for i in range(6):
        outs.append(s.push(feats[:, 4 * i:4 * i + 4]))
        # latency_frames = 8: the pushes at frames 0 and 4 have partial windows and run eagerly
        assert len(s._graphs) == (0 if i < 2 else 1), (i, list(s._graphs))
    outs.append(s.flush())
    assert len(s._graphs) == 1
    assert torch.equal(torch.cat(outs, -1), eager)
    # a second utterance after reset() equals a fresh stream's
    s.reset()
    assert torch.equal(_stream(model, c2, (4,) * 6, stream=s), _bf16(model, c2, (4,) * 6))
    # other weights: the output follows, no stale graph or bf16 image is used
    sd, c_new, ref, e_emu = _oracle_and_emulation(77, 1.1, "c24", 24, 22)
    assert torch.equal(c_new.to(device), c)
    model.load_state_dict(sd)
    s.reset()
    new = _stream(model, c, (4,) * 6, stream=s)
    _within_the_bar(new, ref, e_emu, "graph mode, other weights")
    assert max_abs(new, eager) > 1e-3


# ---- 10. the V1 widths ---------------------------------------------------------------------------------------------
def test_v1_geometry(device):
    """512 channels: 16 frames in pushes of 4 (all inside the latency of 13 frames but the last), then the flush."""
    g = models.HiFiGANGenerator(**synth.HIFIGAN_V1)
    g.load_state_dict(synth_for(g, 11, 1.25))
    g = g.to(device).eval()
    c = synth.synth_input("c", (1, 80, 16), seed=11).to(device)
    s = LookaheadStream(g, use_graph=False, precision="bf16")
    assert (s.latency_samples, s.latency_frames) == (3258, 13)
    assert s.state_bytes == LookaheadStream(g, use_graph=False).state_bytes
    y = _stream(g, c, (4,) * 4, stream=s)
    assert torch.isfinite(y).all() and y.abs().max() > 1e-3
    assert torch.equal(_bf16(g, c, (16,)), y)
