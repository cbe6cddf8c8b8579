"""GPU: streaming the NON-causal HiFi-GAN with a fixed look-ahead (the delayed form of csrc/conv1d_stream.hip,
utils.LookaheadStream) -- the delayed launch against the plain one bit for bit, the streamed generator
against the oracle and the package's own whole-utterance forward, bit-identical audio for every partition, and the
state handling around it."""
import functools

import pytest
import torch

from oracle import torch_cpu
from parallelwavegan_amd import layers, models, ops
from parallelwavegan_amd.layers.causal_conv import lookahead_desc, lookahead_history_columns
from parallelwavegan_amd.utils import LookaheadStream
from parallelwavegan_amd.utils.streaming import to_pcm16
from tests.golden import synth
from tests.util import WAVE_TOL, max_abs, poison_lds, synth_for

pytestmark = pytest.mark.gpu

CHUNKS = (5, 16, 17, 33, 70)  # every column tile of the stream kernel (16 / 32 / 64 columns) and its edges
PIECES = (1, 7, 2, 13, 5, 1, 21)  # chunks shorter than both delays
FUSED = dict(pre_act="leaky_relu", pre_slope=0.1, out_div=3.0)


def _layer(kind, device):
    torch.manual_seed(9)
    cv = layers.Conv1d(24, 40, 5, dilation=3, padding=6) if kind == "conv" else layers.ConvTranspose1d(24, 12, 8, 4, padding=2)
    return cv.to(device), (4 if kind == "up" else 1)


def _rand(gen, *shape):
    return torch.randn(*shape, generator=gen)


def _nan(device, *shape):
    return torch.full(shape, float("nan"), device=device)


# ---- 1. the delayed launch against the plain one -------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["conv", "up"])
def test_no_delay_full_window_equals_the_plain_launch(kind, device):
    cv, s = _layer(kind, device)
    gen = torch.Generator().manual_seed(31)
    h_cols, bias, w = lookahead_history_columns(cv), cv.bias.detach(), cv.packed_weight()
    for n in CHUNKS:
        x, hist = _rand(gen, 2, 24, n).to(device), _rand(gen, 2, 24, h_cols).to(device)
        a1, a2 = (_rand(gen, 2, cv.out_channels, n * s).to(device) for _ in range(2))
        desc = lookahead_desc(cv, 2, n, **FUSED)
        for hist_in in (hist, None):  # (None: start of stream)
            h0, h1 = _nan(device, 2, 24, h_cols), _nan(device, 2, 24, h_cols)
            y0 = ops.conv1d_stream_forward(desc, x, hist_in, h0, w, bias, a1, a2)
            y1 = ops.conv1d_stream_delayed_forward(desc, x, hist_in, h1, w, bias, a1, (None, None), 0, a2, (None, None), 0)
            assert torch.equal(y0, y1) and torch.equal(h0, h1), (kind, n)


@pytest.mark.parametrize("kind", ["conv", "up"])
def test_delayed_addends_equal_host_delayed_addends(kind, device):
    cv, s = _layer(kind, device)
    gen = torch.Generator().manual_seed(32)
    total, d1, d2 = sum(PIECES), 7, 30
    h_cols, bias, w, c_out = lookahead_history_columns(cv), cv.bias.detach(), cv.packed_weight(), cv.out_channels
    x = _rand(gen, 2, 24, total).to(device)
    a1, a2 = (_rand(gen, 2, c_out, total * s).to(device) for _ in range(2))
    # delayed on the host: `delay` zero columns in front
    a1_late = torch.cat([torch.zeros(2, c_out, d1, device=device), a1], -1)
    a2_late = torch.cat([torch.zeros(2, c_out, d2, device=device), a2], -1)
    hist = [[_nan(device, 2, 24, h_cols) for _ in range(2)] for _ in range(2)]          # [entry][ping-pong]
    line1, line2 = ([_nan(device, 2, c_out, d) for _ in range(2)] for d in (d1, d2))
    t, cur = 0, None
    for n in PIECES:
        nxt = 0 if cur is None else 1 - cur
        pick = lambda bufs: (None if cur is None else bufs[cur], bufs[nxt])  # noqa: E731
        xs = x[..., t:t + n].contiguous()
        lo, hi = t * s, (t + n) * s
        desc = lookahead_desc(cv, 2, n, **FUSED)
        y_ref = ops.conv1d_stream_forward(desc, xs, *pick(hist[0]), w, bias, a1_late[..., lo:hi].contiguous(),
                                          a2_late[..., lo:hi].contiguous())
        y = ops.conv1d_stream_delayed_forward(desc, xs, *pick(hist[1]), w, bias, a1[..., lo:hi].contiguous(), pick(line1),
                                              d1, a2[..., lo:hi].contiguous(), pick(line2), d2)
        assert torch.equal(y, y_ref), (kind, t, n)
        assert torch.equal(hist[0][nxt], hist[1][nxt])
        # the delay lines hold the last `delay` columns of concat(zeros, addend so far)
        assert torch.equal(line1[nxt], a1_late[..., hi:hi + d1]) and torch.equal(line2[nxt], a2_late[..., hi:hi + d2])
        cur, t = nxt, t + n


@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("kind", ["conv", "up"])
def test_valid_window_stores_exact_zeros_outside(kind, poison, device):
    cv, s = _layer(kind, device)
    gen = torch.Generator().manual_seed(33)
    h_cols, bias, w, c_out = lookahead_history_columns(cv), cv.bias.detach(), cv.packed_weight(), cv.out_channels
    for n in CHUNKS:
        t_out = n * s
        x, hist = _rand(gen, 2, 24, n).to(device), _rand(gen, 2, 24, h_cols).to(device)
        a1, l1 = _rand(gen, 2, c_out, t_out).to(device), _rand(gen, 2, c_out, 7).to(device)
        desc = lookahead_desc(cv, 2, n, post_act="tanh", **FUSED)

        def run(valid):
            y = _nan(device, 2, c_out, t_out)
            ops.conv1d_stream_delayed_forward(desc, x, hist, _nan(device, 2, 24, h_cols), w, bias, a1,
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


def test_delay_line_buffers_must_be_distinct_and_present(device):
    cv, _ = _layer("conv", device)
    desc = lookahead_desc(cv, 1, 4)
    x, add = torch.zeros(1, 24, 4, device=device), torch.zeros(1, 40, 4, device=device)
    hist, line = torch.zeros(1, 24, 12, device=device), torch.zeros(1, 40, 7, device=device)
    with pytest.raises(RuntimeError, match="distinct"):
        ops.conv1d_stream_delayed_forward(desc, x, None, hist, cv.packed_weight(), None, add, (line, line), 7)
    with pytest.raises(RuntimeError, match="hist_out"):
        ops.conv1d_stream_delayed_forward(desc, x, None, hist, cv.packed_weight(), None, add, (None, None), 7)


# ---- 2. the streamed generator -------------------------------------------------------------------------------------
TINY_FRAMES, TINY_UP, TINY_LATENCY = 23, 24, 182


@functools.lru_cache(maxsize=None)
def _tiny_case(additional=True):
    """(cfg, state dict, c (2, 80, 23) on the CPU, oracle (2, 23 * 24) on the CPU): computed once, never modified."""
    cfg = dict(synth.HIFIGAN_TINY, use_additional_convs=additional)
    sd = synth_for(models.HiFiGANGenerator(**cfg), 21, 1.0)
    c = synth.synth_input("c", (2, 80, TINY_FRAMES), seed=21)
    with torch.no_grad():
        ref = torch_cpu.hifigan_generator(sd, c, **cfg)[:, 0]
    return cfg, sd, c, ref


def _tiny_model(device, additional=True):
    cfg, sd, _, _ = _tiny_case(additional)
    m = models.HiFiGANGenerator(**cfg)
    m.load_state_dict(sd)
    return m.to(device).eval()


def _stream(model, c, pieces, stream=None, **kw):
    """Push c (B, C, T) in ``pieces``, then flush -> (B, T * up); checks the emission length after every push."""
    assert sum(pieces) == c.shape[-1]
    s = stream or LookaheadStream(model, batch=c.shape[0], **kw)
    feats = c.transpose(1, 2).contiguous()
    outs, t, emitted = [], 0, 0
    for n in pieces:
        y = s.push(feats[:, t:t + n])
        t += n
        assert y.shape == (c.shape[0], max(0, t * s.up - s.latency_samples) - emitted), (t, y.shape)
        emitted += y.shape[1]
        outs.append(y)
    assert s.frames_in == c.shape[-1]
    tail = s.flush()
    assert tail.shape[1] == c.shape[-1] * s.up - emitted and s.samples_out == c.shape[-1] * s.up
    assert s.flush().shape == (c.shape[0], 0)
    with pytest.raises(RuntimeError, match="flushed"):
        s.push(feats[:, :1])
    s.close()
    return torch.cat(outs + [tail], -1)


def test_tiny_partitions_are_bit_identical_and_match_oracle_and_forward(device):
    _, _, c_cpu, ref = _tiny_case()
    model, c = _tiny_model(device), _tiny_case()[2].to(device)
    s = LookaheadStream(model, batch=2, use_graph=False)
    assert (s.latency_samples, s.latency_frames, s.up) == (TINY_LATENCY, 8, TINY_UP)
    assert s.state_bytes == 2 * 4 * sum(t.numel() for t in s._halves[0]) > 0
    whole = _stream(model, c, (TINY_FRAMES,), stream=s)
    for pieces in ((1,) * TINY_FRAMES, (3, 1, 7, 2, 5, 5)):
        assert torch.equal(_stream(model, c, pieces, use_graph=False), whole), pieces
    # two lock-step streams equal two single ones
    for b in range(2):
        assert torch.equal(_stream(model, c[b:b + 1], (3, 1, 7, 2, 5, 5), use_graph=False)[0], whole[b])
    with torch.no_grad():
        full = model(c)[:, 0]
    e_oracle, e_forward, e_forward_oracle = max_abs(whole, ref), max_abs(whole, full), max_abs(full, ref)
    print("tiny: stream vs oracle", e_oracle, "stream vs forward", e_forward, "forward vs oracle", e_forward_oracle)
    assert e_oracle <= WAVE_TOL
    assert e_forward <= 2e-5


@pytest.mark.parametrize("frames", [1, 2])
def test_utterance_shorter_than_the_latency(frames, device):
    cfg, sd, c_cpu, _ = _tiny_case()
    c_cpu = c_cpu[..., :frames].contiguous()
    with torch.no_grad():
        ref = torch_cpu.hifigan_generator(sd, c_cpu, **cfg)[:, 0]
    model, c = _tiny_model(device), c_cpu.to(device)
    y = _stream(model, c, (1,) * frames, use_graph=False)  # (every push returns empty: checked in _stream)
    assert y.shape == (2, frames * TINY_UP)
    with torch.no_grad():
        full = model(c)[:, 0]
    print("short", frames, max_abs(y, ref), max_abs(y, full))
    assert max_abs(y, ref) <= WAVE_TOL
    assert max_abs(y, full) <= 2e-5


def test_without_additional_convs(device):
    _, _, c_cpu, ref = _tiny_case(False)
    model, c = _tiny_model(device, False), c_cpu.to(device)
    whole = _stream(model, c, (TINY_FRAMES,), use_graph=False)
    assert torch.equal(_stream(model, c, (3, 1, 7, 2, 5, 5), use_graph=False), whole)
    with torch.no_grad():
        full = model(c)[:, 0]
    print("no additional convs", max_abs(whole, ref), max_abs(whole, full))
    assert max_abs(whole, ref) <= WAVE_TOL
    assert max_abs(whole, full) <= 2e-5


def test_graph_mode(device):
    cfg, _, _, _ = _tiny_case()
    model = _tiny_model(device)
    c = synth.synth_input("c24", (2, 80, 24), seed=22).to(device)
    c2 = synth.synth_input("c24b", (2, 80, 24), seed=23).to(device)
    eager = _stream(model, c, (4,) * 6, use_graph=False)
    s = LookaheadStream(model, batch=2, use_graph=True)
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
    assert torch.equal(_stream(model, c2, (4,) * 6, stream=s), _stream(model, c2, (4,) * 6, use_graph=False))
    # other weights: the output follows, no stale graph is replayed
    model.load_state_dict(synth_for(models.HiFiGANGenerator(**cfg), 77, 1.1))
    s.reset()
    new = _stream(model, c, (4,) * 6, stream=s)
    with torch.no_grad():
        full = model(c)[:, 0]
    assert max_abs(new, full) <= 2e-5
    assert max_abs(new, eager) > 1e-3


def test_push_pcm16_and_normalize_before(device):
    model = _tiny_model(device)
    gen = torch.Generator().manual_seed(17)
    mean, scale = torch.randn(80, generator=gen) * 0.1, 1.0 + 0.1 * torch.rand(80, generator=gen)
    model.register_buffer("mean", mean.to(device))
    model.register_buffer("scale", scale.to(device))
    f = (torch.randn(12, 80, generator=gen) * scale + mean).to(device)
    full = model.inference(f, normalize_before=True).reshape(-1)
    s = LookaheadStream(model, normalize_before=True, use_graph=False)
    y = torch.cat([s.push(f[t:t + 4]) for t in range(0, 12, 4)] + [s.flush()], -1)  # (the flush frames are zeros AFTER
    assert max_abs(y[0], full) <= 2e-5                                               # normalisation)
    s.reset()
    pcm = torch.cat([s.push_pcm16(f[t:t + 4]) for t in range(0, 12, 4)], -1)
    assert pcm.dtype == torch.int16 and pcm.shape == (1, 12 * TINY_UP - TINY_LATENCY)
    assert torch.equal(pcm, to_pcm16(y[:, :pcm.shape[1]]))


def test_v1_geometry(device):
    """512 channels: 16 frames in pushes of 4 (all inside the latency of 13 frames but the last), then the flush."""
    cfg = synth.HIFIGAN_V1
    g = models.HiFiGANGenerator(**cfg)
    sd = synth_for(g, 11, 1.25)
    g.load_state_dict(sd)
    g = g.to(device).eval()
    c_cpu = synth.synth_input("c", (1, 80, 16), seed=11)
    with torch.no_grad():
        ref = torch_cpu.hifigan_generator(sd, c_cpu, **cfg)[:, 0]
    c = c_cpu.to(device)
    s = LookaheadStream(g, use_graph=False)
    assert (s.latency_samples, s.latency_frames) == (3258, 13)
    y = _stream(g, c, (4,) * 4, stream=s)
    assert torch.equal(_stream(g, c, (16,), use_graph=False), y)
    err = max_abs(y, ref)
    print("v1 stream vs oracle", err)
    assert err <= WAVE_TOL
