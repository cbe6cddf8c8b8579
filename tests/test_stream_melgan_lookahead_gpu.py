"""GPU: streaming the NON-causal (multi-band) MelGAN with a fixed look-ahead (the mirrored form of
csrc/conv1d_stream.hip, utils.MelGANLookaheadStream) -- one reflect-padded layer fed chunk by chunk
with the utterance's edges at chosen places against the float64 reflect-padded convolution, the streamed generators
against the whole-utterance forward and the oracle, bit-identical audio for every partition, graph replay, and the
reference golden of the multi-band model through the stateful PQMF synthesis."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import torch_cpu
from parallelwavegan_amd import layers, models, ops
from parallelwavegan_amd.layers.causal_conv import mirrored_desc
from parallelwavegan_amd.utils import MelGANLookaheadStream
from tests.golden import synth
from tests.util import WAVE_TOL, load_golden, max_abs, poison_lds, synth_for

pytestmark = pytest.mark.gpu

# the multi-band generator of the reference golden (tests/test_pwg_melgan_gpu.py, the same fixture)
MB_G = dict(in_channels=80, out_channels=4, kernel_size=7, channels=384, upsample_scales=[8, 4, 2],
            stack_kernel_size=3, stacks=4, use_weight_norm=True, use_causal_conv=False)
FORWARD_TOL = 2e-5  # tests/test_stream_lookahead_gpu.py: a look-ahead stream (and its delayed layers) against `forward`
SLOPE = 0.2


def _nan(device, *shape):
    return torch.full(shape, float("nan"), device=device)


# ---- 1. one layer through ops ----------------------------------------------------------------------------------------
def _feed(cv, stream, d_in, t_len, pieces, device, post_act=None):
    """``stream`` (2, C, L): the layer's raw input, the utterance at [d_in, d_in + t_len), anything around it; fed in
    ``pieces`` through the mirrored launch with NaN-filled state halves and outputs -> (2, C_out, L)."""
    assert sum(pieces) == stream.shape[-1]
    p, h_cols = cv.padding, 2 * cv.padding
    hist = [_nan(device, 2, cv.in_channels, h_cols) for _ in range(2)]
    w, bias = cv.packed_weight(), cv.bias.detach()
    outs, t, cur = [], 0, None
    for n in pieces:
        nxt = 0 if cur is None else 1 - cur
        desc = mirrored_desc(cv, 2, n, pre_act="leaky_relu", pre_slope=SLOPE, **({"post_act": post_act} if post_act else {}))
        y = _nan(device, 2, cv.out_channels, n)
        lo, hi = d_in - t, d_in + t_len - t
        ops.conv1d_stream_mirrored_forward(desc, stream[..., t:t + n].contiguous(), None if cur is None else hist[cur],
                                           hist[nxt], w, bias, (lo, hi),
                                           (min(max(lo + p, 0), n), min(max(hi + p, 0), n)), out=y)
        # the history stays raw: the last columns of the input, zeros before the stream
        raw = torch.cat([torch.zeros(2, cv.in_channels, h_cols, device=device), stream[..., :t + n]], -1)
        assert torch.equal(hist[nxt], raw[..., raw.shape[-1] - h_cols:]), (t, n)
        outs.append(y)
        cur, t = nxt, t + n
    return torch.cat(outs, -1)


def _split(total, head, step):
    """``head`` then pieces of ``step`` columns (the last one shorter) up to ``total``."""
    rest = total - sum(head)
    assert rest >= 0
    return tuple(head) + (step,) * (rest // step) + ((rest % step,) if rest % step else ())


@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("k,d", [(7, 1), (3, 9), (3, 27)])
def test_mirrored_layer_equals_the_reflect_padded_convolution(k, d, poison, device):
    torch.manual_seed(9)
    p = (k - 1) * d // 2
    cv = layers.Conv1d(24, 40, k, dilation=d, padding=p, pad_mode="reflect").to(device)
    post = "tanh" if k == 7 else None
    gen = torch.Generator().manual_seed(41 + d)
    # (name, d_in, utterance length, pieces of the d_in + T + p columns the stream needs)
    scenarios = [
        ("left edge in the chunk", 5, p + 9, lambda n: _split(n, (p + 8,), 6)),
        ("left edge in the history", 5, p + 9, lambda n: _split(n, (5, 1, 2), 3)),
        ("left edge at a 16-column tile boundary", 16, p + 12, lambda n: _split(n, (20,), 7)),
        ("right edge in the history, last push one column", 4, p + 6, lambda n: _split(n - 3, (3,), 5) + (1, 1, 1)),
        ("both edges inside one window", 3, p + 1, lambda n: (n,)),
        ("more than 64 columns: several column tiles see an edge", 10, 70, lambda n: _split(n, (100,), 33)),
    ]
    w64, b64 = cv.weight.detach().double().cpu(), cv.bias.detach().double().cpu()
    for name, d_in, t_len, pieces_of in scenarios:
        total = max(d_in + t_len + p, 101 if t_len == 70 else 0)
        x = torch.randn(2, 24, t_len, generator=gen)
        stream = 7.0 + torch.randn(2, 24, total, generator=gen)  # what lies around the utterance is never read ...
        stream[..., d_in:d_in + t_len] = x
        ref = F.conv1d(F.pad(F.leaky_relu(x.double(), SLOPE), (p, p), mode="reflect"), w64, b64, dilation=d)
        if post:
            ref = torch.tanh(ref)
        pieces = pieces_of(total)
        if poison:
            with poison_lds():
                y = _feed(cv, stream.to(device), d_in, t_len, pieces, device, post)
        else:
            y = _feed(cv, stream.to(device), d_in, t_len, pieces, device, post)
        body = y[..., d_in + p:d_in + p + t_len]
        err = max_abs(body, ref)
        print(f"k={k} d={d} {name}: pieces {pieces} err {err:.3g}")
        assert err <= FORWARD_TOL, name
        outside = torch.cat([y[..., :d_in + p], y[..., d_in + p + t_len:]], -1)  # ... and stored as exact zeros
        assert outside.numel() and torch.equal(outside, torch.zeros_like(outside)), name


def test_mirrored_forward_checks_its_buffers(device):
    cv = layers.Conv1d(24, 40, 7, padding=3, pad_mode="reflect").to(device)
    x, hist = torch.zeros(1, 24, 4, device=device), torch.zeros(1, 24, 6, device=device)
    with pytest.raises(RuntimeError, match="distinct"):
        ops.conv1d_stream_mirrored_forward(mirrored_desc(cv, 1, 4), x, hist, hist, cv.packed_weight())
    with pytest.raises(RuntimeError, match="pad_mode"):
        ops.conv1d_stream_mirrored_forward(ops.make_conv_desc(1, 24, 40, 4, 4, 7, pad_left=6), x, None, hist,
                                           cv.packed_weight())


# ---- 2. the streamed generators --------------------------------------------------------------------------------------
TINY = dict(synth.MELGAN_CAUSAL, use_causal_conv=False)  # channels 64, scales [4, 2, 2], 2 stacks: 16 samples a frame
TINY_MB = dict(in_channels=80, out_channels=4, kernel_size=7, channels=32, upsample_scales=[3, 2], stack_kernel_size=3,
               stacks=3)  # an odd stride, dilations 1, 3, 9, 4 sub-bands: 24 samples a frame
CASES = {"tiny": (TINY, 90, 6, 16), "tiny_mb": (TINY_MB, 65 * 4 + 32, 13, 24)}  # cfg, latency, settle_frames, up
FRAMES = 16


@functools.lru_cache(maxsize=None)
def _case(name):
    """(cfg, state dict, c (16, 80, FRAMES) on the CPU, oracle (16, FRAMES * up) on the CPU): computed once, never
    modified."""
    cfg = CASES[name][0]
    sd = synth_for(models.MelGANGenerator(**cfg), 21, synth.MELGAN_G_SCALE)
    c = synth.synth_input("c", (16, 80, FRAMES), seed=21)
    with torch.no_grad():
        ref = torch_cpu.melgan_generator(sd, c, **cfg)
        ref = torch_cpu.pqmf_synthesis(ref)[:, 0] if cfg["out_channels"] > 1 else ref[:, 0]
    return cfg, sd, c, ref


def _model(name, device):
    cfg, sd, _, _ = _case(name)
    m = models.MelGANGenerator(**cfg)
    m.load_state_dict(sd)
    m = m.to(device).eval()
    if cfg["out_channels"] > 1:
        m.pqmf = layers.PQMF(subbands=cfg["out_channels"]).to(device)
    return m


def _whole(model, c):
    with torch.no_grad():
        y = model(c)
        return (model.pqmf.synthesis(y) if model.pqmf is not None else y)[:, 0]


def _stream(model, c, pieces, stream=None, **kw):
    """Push c (B, C, T) in ``pieces``, then flush -> (B, T * up); checks the emission length after every push."""
    assert sum(pieces) == c.shape[-1]
    s = stream or MelGANLookaheadStream(model, batch=c.shape[0], **kw)
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


RANDOM = (3, 1, 5, 2, 4, 1)


@pytest.mark.parametrize("name", list(CASES))
def test_partitions_are_bit_identical_and_match_forward_and_oracle(name, device):
    _, latency, settle, up = CASES[name]
    _, _, c_cpu, ref = _case(name)
    model, c = _model(name, device), c_cpu.to(device)
    s = MelGANLookaheadStream(model, batch=2, use_graph=False)
    assert (s.latency_samples, s.latency_frames, s.settle_frames, s.min_frames, s.up) == \
        (latency, -(-latency // up), settle, 4, up)
    assert s.state_bytes == 2 * 4 * sum(t.numel() for t in s._halves[0]) > 0
    whole = _stream(model, c[:2], (FRAMES,), stream=s)
    for pieces in ((1,) * FRAMES, RANDOM):
        assert torch.equal(_stream(model, c[:2], pieces, use_graph=False), whole), pieces
    # reset(), then a second utterance: the first one again
    s.reset()
    assert torch.equal(_stream(model, c[:2], RANDOM, stream=s), whole)
    full = _whole(model, c[:2])
    e_forward, e_oracle = max_abs(whole, full), max_abs(whole, ref[:2])
    print(name, "stream vs forward", e_forward, "stream vs oracle", e_oracle, "forward vs oracle", max_abs(full, ref[:2]))
    assert e_forward <= FORWARD_TOL
    assert e_oracle <= WAVE_TOL


@pytest.mark.parametrize("name", list(CASES))
def test_sixteen_lock_step_streams_equal_sixteen_single_ones(name, device):
    model, c = _model(name, device), _case(name)[2].to(device)
    together = _stream(model, c, RANDOM, use_graph=False)
    single = MelGANLookaheadStream(model, batch=1, use_graph=False)
    for b in range(16):
        single.reset()
        assert torch.equal(_stream(model, c[b:b + 1], (FRAMES,), stream=single)[0], together[b]), b


@pytest.mark.parametrize("name", list(CASES))
def test_graph_replay_equals_eager(name, device):
    _, _, settle, _ = CASES[name]
    model = _model(name, device)
    frames = 4 * (-(-settle // 4) + 3)
    c = synth.synth_input("c_graph", (2, 80, frames), seed=22).to(device)
    pieces = (4,) * (frames // 4)
    eager = _stream(model, c, pieces, use_graph=False)
    s = MelGANLookaheadStream(model, batch=2, use_graph=True)
    feats = c.transpose(1, 2).contiguous()
    outs = []
    for i in range(len(pieces)):
        outs.append(s.push(feats[:, 4 * i:4 * i + 4]))
        # a push replays a graph only once settle_frames went before it
        assert len(s._graphs) == (0 if 4 * i < settle else 1), (i, list(s._graphs))
    outs.append(s.flush())
    assert len(s._graphs) == 1
    assert torch.equal(torch.cat(outs, -1), eager)
    s.reset()
    assert torch.equal(_stream(model, c, pieces, stream=s), eager)
    assert max_abs(eager, _whole(model, c)) <= FORWARD_TOL


def test_an_utterance_too_short_for_reflection(device):
    model = _model("tiny", device)
    s = MelGANLookaheadStream(model, use_graph=False)
    c = _case("tiny")[2][:1].to(device)
    feats = c.transpose(1, 2).contiguous()
    for t in range(3):
        assert s.push(feats[:, t:t + 1]).shape == (1, 0)
    with pytest.raises(RuntimeError, match="at least 4"):
        s.flush()
    # exactly the minimum: both mirrors of the first layer fall in one window
    s.reset()
    short = c[..., :4].contiguous()
    assert max_abs(_stream(model, short, (2, 2), stream=s), _whole(model, short)) <= FORWARD_TOL


def test_push_pcm16_and_normalize_before(device):
    from parallelwavegan_amd.utils.streaming import to_pcm16

    model = _model("tiny_mb", device)
    gen = torch.Generator().manual_seed(17)
    mean, scale = torch.randn(80, generator=gen) * 0.1, 1.0 + 0.1 * torch.rand(80, generator=gen)
    model.register_buffer("mean", mean.to(device))
    model.register_buffer("scale", scale.to(device))
    f = (torch.randn(20, 80, generator=gen) * scale + mean).to(device)  # 480 samples, past the latency of 292
    full = model.inference(f, normalize_before=True).reshape(-1)
    s = MelGANLookaheadStream(model, normalize_before=True, use_graph=False)
    y = torch.cat([s.push(f[t:t + 4]) for t in range(0, 20, 4)] + [s.flush()], -1)
    assert max_abs(y[0], full) <= FORWARD_TOL
    s.reset()
    pcm = torch.cat([s.push_pcm16(f[t:t + 4]) for t in range(0, 20, 4)], -1)
    assert pcm.dtype == torch.int16 and pcm.shape == (1, 20 * 24 - s.latency_samples)
    assert torch.equal(pcm, to_pcm16(y[:, :pcm.shape[1]]))


# ---- 3. the reference golden of the multi-band model -----------------------------------------------------------------
def test_multi_band_golden_through_the_stream(device):
    gold = load_golden("mb_melgan_v2")
    seed = int(gold["meta"][0])
    g = models.MelGANGenerator(**MB_G)
    g.load_state_dict(synth.synth_state_dict(g.state_dict(), seed=seed, g_scale=synth.MELGAN_G_SCALE))
    g = g.to(device).eval()
    g.pqmf = layers.PQMF().to(device)
    c = synth.synth_input("c", (2, 80, 24), seed=seed)[:1].to(device)
    s = MelGANLookaheadStream(g, use_graph=False)
    assert (s.latency_samples, s.up) == (672 * 4 + 32, 256)  # [8, 4, 2], 4 stacks: 672 sub-band columns, + the PQMF's 32
    y = _stream(g, c, (5, 7, 1, 11), stream=s)
    err = max_abs(y[0], gold["g_y_inference"].reshape(-1))
    print("mb_melgan_v2 golden through the stream", err)
    assert err <= WAVE_TOL
