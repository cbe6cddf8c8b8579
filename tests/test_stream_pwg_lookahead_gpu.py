"""GPU: streaming the standard NON-causal Parallel WaveGAN with a fixed look-ahead -- the gated layer in delayed form
(csrc/wavenet_stream.hip), the upsampler stage with a valid window (pwg_stretch_conv_stream_delayed), the delay line
(pwg_delay_line_forward) and utils.PWGLookaheadStream end to end: parity with float64 / the reference
golden / the whole-utterance forward, and bit identity across partitions, batch and graph replay."""
import copy
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import torch_cpu
from parallelwavegan_amd import _lib, models, ops, utils
from parallelwavegan_amd.layers.causal_conv import lookahead_window
from parallelwavegan_amd.layers.residual_block import WaveNetResidualBlock
from parallelwavegan_amd.ops import _ptr, _stream
from tests.golden import synth
from tests.util import WAVE_TOL, load_golden, max_abs, poison_lds, synth_for

pytestmark = pytest.mark.gpu

DILATIONS = (1, 4, 512)
B, T = 2, 1200
PARTITIONS = ((1, 63, 64, 65, 7, 1000), (1200,), (3,) * 400)
SKIP_SCALE = 0.5
EXTRA = 37  # the second c_delay of a dilation is d + EXTRA: an unaligned read of the conditioning line
SMALL = dict(layers=6, stacks=2, aux_context_window=2, upsample_params={"upsample_scales": [4, 4]})  # latency 66
DEEP = dict(layers=10, stacks=1, aux_context_window=2, upsample_params={"upsample_scales": [4, 4]})  # latency 1075


def _rel(a, b):
    """The relative-to-max measure of tests/test_wavenet_layer_gpu.py."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-12)


# ---- the layer ---------------------------------------------------------------------------------------------------------
_LAYER = {}


def _effective_weight(cv):
    v, g = cv.weight_v.detach().double(), cv.weight_g.detach().double()
    return v * (g / v.reshape(v.shape[0], -1).norm(dim=1).reshape(-1, 1, 1))


def _new_block(d):
    blk = WaveNetResidualBlock(dilation=d)
    for cv in blk.fused_convs():
        cv.apply_weight_norm()
    return blk


def _layer_case(d):
    """Seeded non-causal block (weight-normed, non-zero biases), inputs and the float64 evaluation of the block's formula
    (layers/residual_block.py:102-140 of the reference) on the zero-padded input, once per dilation on the CPU.  The
    stream's output column tau is the formula's column tau - d; the conditioning the stream reads ``c_delay`` late is the
    formula's ``c`` shifted by ``c_delay - d`` (zeros in front); the skip sum is read d late, i.e. aligned."""
    if d not in _LAYER:
        torch.manual_seed(2000 + d)
        blk = _new_block(d)
        with torch.no_grad():
            for p in blk.parameters():
                p.add_(0.1 * torch.randn_like(p))
        g = torch.Generator().manual_seed(d)
        x, c, skips = (torch.randn(B, ch, T, generator=g) for ch in (64, 80, 64))
        w_d, w_a, w_s, w_o = (_effective_weight(cv) for cv in blk.fused_convs())
        b_d, b_s, b_o = (cv.bias.detach().double() for cv in (blk.conv, blk.conv1x1_skip, blk.conv1x1_out))
        xd = x.double()
        conv = F.conv1d(xd, w_d, b_d, dilation=d, padding=d)
        refs = {}
        for c_delay in (d, d + EXTRA):
            c_shift = F.pad(c.double(), (c_delay - d, 0))[..., :T]
            z = conv + F.conv1d(c_shift, w_a)
            gt = torch.tanh(z[:, :64]) * torch.sigmoid(z[:, 64:])
            refs[c_delay] = dict(x=(F.conv1d(gt, w_o, b_o) + xd) * math.sqrt(0.5),
                                 s=(F.conv1d(gt, w_s, b_s) + skips.double()) * SKIP_SCALE,
                                 s0=F.conv1d(gt, w_s, b_s) * SKIP_SCALE)
        _LAYER[d] = dict(state=blk.state_dict(), x=x, c=c, skips=skips, refs=refs)
    return _LAYER[d]


def _block(d, device):
    blk = _new_block(d)
    blk.load_state_dict(_layer_case(d)["state"])
    return blk.to(device).eval()


def _nan(shape, device):
    return [torch.full(shape, float("nan"), device=device) for _ in range(2)]


def _stream_layer(blk, x, c, skips, parts, c_delay, check_state=False):
    """Stream (x, c, skips) through ``blk`` in pieces -> (x_out, skips_out), d columns late.  Every state buffer starts as
    NaN, so a start-of-stream read of a state (or an unwritten part of one) shows in the output.  The conditioning line
    holds c_delay + 5 columns (more than the layer needs: it is shared in a generator)."""
    nb, d, dev = x.shape[0], blk.conv.dilation, x.device
    hist, sline, cline = _nan((nb, 64, 2 * d), dev), _nan((nb, 64, d), dev), _nan((nb, 80, c_delay + 5), dev)
    want = [torch.zeros_like(t[0]) for t in (hist, sline, cline)]
    xs, ss, pos, cur = [], [], 0, 0
    for i, n in enumerate(parts):
        xp, cp = x[:, :, pos:pos + n].contiguous(), c[:, :, pos:pos + n].contiguous()
        sp = None if skips is None else skips[:, :, pos:pos + n].contiguous()
        first = i == 0
        xo, so = blk.lookahead_forward(xp, cp, None if first else cline[cur], c_delay,
                                       (None if first else hist[cur], hist[1 - cur]), sp,
                                       (None if first else sline[cur], sline[1 - cur]),
                                       lookahead_window(d, 1, n, pos), skip_scale=SKIP_SCALE)
        assert ops.delay_line_forward(cp, None if first else cline[cur], cline[1 - cur]) is None
        cur = 1 - cur
        if check_state:
            news = (xp, sp, cp)
            for k, (buf, new) in enumerate(zip((hist, sline, cline), news)):
                if new is None:
                    continue
                want[k] = torch.cat([want[k], new], -1)[..., -want[k].shape[-1]:]
                assert torch.equal(buf[cur], want[k]), (k, i, n)
        xs.append(xo)
        ss.append(so)
        pos += n
    assert pos == x.shape[-1]
    return torch.cat(xs, -1), torch.cat(ss, -1)


_STREAMED = {}


def _streamed(d, c_delay, device):
    """Every partition of the layer case streamed once (states checked after every piece), shared by the tests."""
    if (d, c_delay) not in _STREAMED:
        case, blk = _layer_case(d), _block(d, device)
        x, c, skips = (case[k].to(device) for k in ("x", "c", "skips"))
        _STREAMED[d, c_delay] = [_stream_layer(blk, x, c, skips, parts, c_delay, check_state=True) for parts in PARTITIONS]
    return _STREAMED[d, c_delay]


def _check_against_oracle(d, got_x, got_s, ref_x, ref_s, what):
    """Columns [0, d) are in front of the utterance: exact zeros.  Column tau >= d is the formula's column tau - d."""
    for name, got, want in (("x", got_x, ref_x), ("skips", got_s, ref_s)):
        assert torch.isfinite(got).all(), (name, what)
        assert float(got[..., :d].abs().max()) == 0.0, (name, what)
        r = _rel(got[..., d:], want[..., :T - d])
        print(f"d={d} {what} {name}: rel {r:.3e}")
        assert r <= 3e-5, (name, what, r)


@pytest.mark.parametrize("extra", [0, EXTRA])
@pytest.mark.parametrize("d", DILATIONS)
def test_layer_matches_float64_oracle(d, extra, device):
    """Figures on an MI355X (relative to max, bound 3e-5): see DESIGN.md s11.6."""
    case = _layer_case(d)
    ref = case["refs"][d + extra]
    for parts, (xo, so) in zip(PARTITIONS, _streamed(d, d + extra, device)):
        _check_against_oracle(d, xo, so, ref["x"], ref["s"], f"c_delay={d + extra} pieces={len(parts)}")
    # without a skip input (the first layer of a generator)
    blk = _block(d, device)
    x, c = (case[k].to(device) for k in ("x", "c"))
    xo, so = _stream_layer(blk, x, c, None, PARTITIONS[0], d + extra)
    _check_against_oracle(d, xo, so, ref["x"], ref["s0"], f"c_delay={d + extra} no skips")
    assert torch.equal(xo, _streamed(d, d + extra, device)[0][0])


@pytest.mark.parametrize("d", DILATIONS)
def test_layer_under_poisoned_lds(d, device):
    case, blk = _layer_case(d), _block(d, device)
    x, c, skips = (case[k].to(device) for k in ("x", "c", "skips"))
    with poison_lds():
        xo, so = _stream_layer(blk, x, c, skips, PARTITIONS[0], d + EXTRA)
    ref_x, ref_s = _streamed(d, d + EXTRA, device)[0]
    assert torch.equal(xo, ref_x) and torch.equal(so, ref_s)


@pytest.mark.parametrize("d", DILATIONS)
def test_layer_partitions_and_batch_are_bit_identical(d, device):
    case, blk = _layer_case(d), _block(d, device)
    x, c, skips = (case[k].to(device) for k in ("x", "c", "skips"))
    for c_delay in (d, d + EXTRA):
        outs = _streamed(d, c_delay, device)  # (also: every state after every piece == last columns of the concat)
        for xo, so in outs[1:]:
            assert torch.equal(xo, outs[0][0]) and torch.equal(so, outs[0][1])
        for b in range(B):  # lock step == single streams
            xo, so = _stream_layer(blk, x[b:b + 1], c[b:b + 1], skips[b:b + 1], PARTITIONS[0], c_delay)
            assert torch.equal(xo, outs[0][0][b:b + 1]) and torch.equal(so, outs[0][1][b:b + 1])


def test_layer_valid_windows_store_exact_zeros(device):
    d, n = 4, 200
    case, blk = _layer_case(d), _block(d, device)
    x, c, skips = (case[k][:, :, :n].contiguous().to(device) for k in ("x", "c", "skips"))
    hist, sline = _nan((B, 64, 2 * d), device), _nan((B, 64, d), device)

    def run(valid):
        return blk.lookahead_forward(x, c, None, d, (None, hist[0]), skips, (None, sline[0]), valid, skip_scale=SKIP_SCALE)

    full_x, full_s = run(None)
    for lo, hi in ((0, n), (5, n), (0, 131), (67, 70), (64, 128), (50, 50), (n, n)):
        xo, so = run((lo, hi))
        for got, full in ((xo, full_x), (so, full_s)):
            assert torch.equal(got[..., lo:hi], full[..., lo:hi]), (lo, hi)
            assert float(got[..., :lo].abs().sum()) == 0.0 and float(got[..., hi:].abs().sum()) == 0.0, (lo, hi)


def test_layer_refuses_aliased_buffers(device):
    d, n = 4, 16
    case, blk = _layer_case(d), _block(d, device)
    x, c, skips = (case[k][:, :, :n].contiguous().to(device) for k in ("x", "c", "skips"))
    h, s = _nan((B, 64, 2 * d), device), _nan((B, 64, d), device)
    with pytest.raises(RuntimeError, match="distinct"):
        blk.lookahead_forward(x, c, None, d, (h[0], h[0]), skips, (None, s[0]))
    with pytest.raises(RuntimeError, match="skip_line_in and skip_line_out must be distinct"):
        blk.lookahead_forward(x, c, None, d, (None, h[0]), skips, (s[0], s[0]))
    with pytest.raises(RuntimeError, match="needs skip_line_out"):
        ops.wavenet_stream_delayed_forward(blk.fused_desc(B, n), x, c, None, d, skips, (None, None), None, h[0],
                                           blk.stream_image(), None, None, None)
    short = torch.zeros(B, 80, d - 1, device=device)
    with pytest.raises(RuntimeError, match="conditioning line"):
        blk.lookahead_forward(x, c, short, d, (None, h[0]), skips, (None, s[0]))
    # skips_out aliasing skips: the wrapper always allocates, so ask the entry point itself
    desc, out = blk.fused_desc(B, n), torch.empty_like(x)
    rc = _lib.lib().pwg_wavenet_stream_delayed_forward(
        ctypes.byref(desc), _ptr(x), _ptr(c), None, 0, d, _ptr(skips), None, _ptr(s[0]), None, _ptr(h[0]),
        _ptr(blk.stream_image()), None, None, None, 0, n, _ptr(out), _ptr(skips), _stream())
    assert rc != 0 and "alias" in _lib.lib().pwg_last_error().decode()


# ---- the upsampler stage -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [4, 3])
@pytest.mark.parametrize("act", [None, "leaky_relu"])
def test_stretch_conv_stream_delayed(scale, act, device):
    Tm = 37
    g = torch.Generator().manual_seed(scale)
    x = torch.randn(2, 80, Tm, generator=g).to(device)
    w = (torch.randn(1, 1, 1, 2 * scale + 1, generator=g) / (2 * scale + 1)).to(device)
    hin = torch.randn(2, 80, 2, generator=g).to(device)
    n_out = Tm * scale
    for h_in in (None, hin):
        h0, h1 = _nan((2, 80, 2), device)
        ref = ops.stretch_conv_stream(x, h_in, h0, w, scale, 1, act, 0.2)
        assert torch.equal(ops.stretch_conv_stream_delayed(x, h_in, h1, w, scale, 1, act, 0.2), ref)  # valid=None: full
        assert torch.equal(h0, h1)
        for lo, hi in ((0, n_out), (scale, n_out), (0, n_out - scale), (5, 9), (7, 7), (n_out, n_out)):
            h1.fill_(float("nan"))
            y = ops.stretch_conv_stream_delayed(x, h_in, h1, w, scale, 1, act, 0.2, (lo, hi))
            assert torch.equal(y[..., lo:hi], ref[..., lo:hi]) and torch.equal(h0, h1), (lo, hi)
            assert float(y[..., :lo].abs().sum()) == 0.0 and float(y[..., hi:].abs().sum()) == 0.0, (lo, hi)
    h = torch.zeros(2, 80, 2, device=device)
    with pytest.raises(RuntimeError, match="distinct"):
        ops.stretch_conv_stream_delayed(x, h, h, w, scale)
    with pytest.raises(RuntimeError, match="freq_kernel"):
        ops.stretch_conv_stream_delayed(x, None, h, torch.zeros(3 * (2 * scale + 1), device=device), scale, freq_kernel=3)


# ---- the delay line ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,L", [(3, 7), (7, 7), (300, 7), (1, 852), (1000, 852)])
def test_delay_line(n, L, device):
    g = torch.Generator().manual_seed(n + L)
    x, line = torch.randn(2, 5, n, generator=g).to(device), torch.randn(2, 5, L, generator=g).to(device)
    for line_in in (None, line):
        cat = torch.cat([torch.zeros_like(line) if line_in is None else line_in, x], -1)
        for delayed in (False, True):
            out = torch.full((2, 5, L), float("nan"), device=device)
            y = ops.delay_line_forward(x, line_in, out, delayed=delayed)
            assert torch.equal(out, cat[..., -L:])
            assert (y is None) if not delayed else torch.equal(y, cat[..., :n])
    with pytest.raises(RuntimeError, match="distinct"):
        ops.delay_line_forward(x, line, line)


# ---- the generator -----------------------------------------------------------------------------------------------------
def _model(cfg, seed, device):
    m = models.ParallelWaveGANGenerator(**cfg)
    sd = synth_for(m, seed, 1.0)
    m.load_state_dict(sd)
    return m.to(device).eval(), sd


def _stream_all(stream, frames, noise, parts):
    """frames (B, C, n) and noise (B, 1, n * up) through ``stream`` in pieces, then the flush -> (B, n * up).  The
    per-push sample counts follow the formula."""
    up, ys, pos, lat = stream.up, [], 0, stream.latency_samples
    for n in parts:
        ys.append(stream.push(frames[:, :, pos:pos + n].transpose(1, 2), noise[:, 0, pos * up:(pos + n) * up]))
        assert ys[-1].shape == (frames.shape[0], max(0, (pos + n) * up - lat) - max(0, pos * up - lat)), (pos, n)
        pos += n
    assert pos == frames.shape[-1] and stream.samples_out == max(0, pos * up - lat)
    ys.append(stream.flush())
    assert ys[-1].shape[1] == min(lat, pos * up) and stream.samples_out == pos * up
    assert stream.flush().shape == (frames.shape[0], 0)
    return torch.cat(ys, -1)


def test_stream_matches_oracle_and_inference(device):
    m, sd = _model(SMALL, 41, device)
    frames = synth.synth_input("c", (2, 80, 18), seed=41)
    z = synth.synth_input("z", (2, 1, 18 * 16), seed=41)
    want = torch_cpu.pwg_generator(sd, z, F.pad(frames, (2, 2), mode="replicate"), **SMALL)
    s = utils.PWGLookaheadStream(m, batch=2, use_graph=False)
    assert (s.latency_samples, s.latency_frames) == (66, 5)
    outs = []
    for parts in ((1, 7, 2, 8), (18,), (1,) * 18):
        s.reset()
        outs.append(_stream_all(s, frames.to(device), z.to(device), parts))
        assert (s.frames_in, s.frames_out, s.samples_out) == (18, 18, 288)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    err = max_abs(outs[0].unsqueeze(1), want)
    print(f"small generator: max abs vs the float oracle {err:.3e}")
    assert err <= WAVE_TOL
    with torch.no_grad():
        for b in range(2):
            own = m.inference(frames[b].t().to(device), x=z[b].t().to(device))  # (T, 1)
            assert max_abs(outs[0][b], own[:, 0]) <= WAVE_TOL
    with pytest.raises(RuntimeError, match="flushed"):
        s.push(frames[:, :, :1].transpose(1, 2))


def test_stream_v1_matches_reference_golden(device):
    gold = load_golden("pwg_v1")
    frames, seed = (int(v) for v in gold["meta"])
    m = models.ParallelWaveGANGenerator()
    m.load_state_dict(synth.synth_state_dict(m.state_dict(), seed=seed, g_scale=synth.PWG_G_SCALE))
    m = m.to(device).eval()
    c = synth.synth_input("c", (1, 80, frames + 4), seed=seed)[:, :, 2:-2]
    z = synth.synth_input("z", (1, 1, frames * 256), seed=seed)
    s = utils.PWGLookaheadStream(m, use_graph=False)
    assert (s.latency_samples, s.latency_frames) == (3921, 16) and frames > 16
    y = _stream_all(s, c.to(device), z.to(device), (3, 9, 1, 40, frames - 53))
    err = max_abs(y[0], gold["g_y_inference"][:, 0])
    print(f"parallel_wavegan.v1: max abs vs the reference golden {err:.3e}")
    assert err <= WAVE_TOL


def test_stream_one_frame_utterance(device):
    m, _ = _model(SMALL, 41, device)
    frame = synth.synth_input("c", (1, 80, 1), seed=7)
    z = synth.synth_input("z", (1, 1, 16), seed=7)
    s = utils.PWGLookaheadStream(m, use_graph=True)
    assert s.flush().shape == (1, 0)  # nothing pushed yet
    assert s.push(frame[0].t(), z[0, 0]).shape == (1, 0)
    y = s.flush()
    assert y.shape == (1, 16)
    with torch.no_grad():
        own = m.inference(frame[0].t().to(device), x=z[0].t().to(device))
    assert max_abs(y[0], own[:, 0]) <= WAVE_TOL


def test_stream_deep_dilations_end_to_end(device):
    m, _ = _model(DEEP, 77, device)
    n, up = 80, 16
    frames = synth.synth_input("c", (2, 80, n), seed=77).to(device)
    z = synth.synth_input("z", (2, 1, n * up), seed=77).to(device)
    s = utils.PWGLookaheadStream(m, batch=2, use_graph=False)
    assert (s.latency_samples, s.latency_frames) == (1075, 68)
    assert s.state_bytes == 2 * 4 * 2 * (80 * 4 + 2 * 80 * 2 + 52 + 80 * 1023 + 64 * 2 * 1023 + 64 * (1023 - 1))
    outs = []
    for parts in ((1,) * n, (n,), (3, 1, 17, 59)):
        s.reset()
        outs.append(_stream_all(s, frames, z, parts))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    s.reset()
    assert torch.equal(_stream_all(s, frames, z, (3, 1, 17, 59)), outs[0])  # reset() and a second pass
    single = utils.PWGLookaheadStream(m, batch=1, use_graph=False)
    for b in range(2):
        single.reset()
        assert torch.equal(_stream_all(single, frames[b:b + 1], z[b:b + 1], (3, 1, 17, 59)), outs[0][b:b + 1])
    with torch.no_grad():
        whole = m(z, F.pad(frames, (2, 2), mode="replicate"))
    err = max_abs(outs[0].unsqueeze(1), whole)
    print(f"deep dilations: max abs vs the whole-utterance forward {err:.3e}")
    assert torch.isfinite(outs[0]).all() and err <= WAVE_TOL


def test_stream_graph_replay_is_bit_identical_to_eager(device):
    m, _ = _model(SMALL, 41, device)
    sizes = (2, 2, 2, 2, 2, 2, 2, 3, 2)  # 3 eager start-up pushes (6 >= latency_frames 5), then A -> B -> A ..., 3, back
    total = sum(sizes)
    frames = synth.synth_input("c", (1, 80, total + 4), seed=5).to(device)
    z = synth.synth_input("z", (1, 1, (total + 4) * 16), seed=5).to(device)
    old = copy.deepcopy(m)
    sg, se = utils.PWGLookaheadStream(m, use_graph=True), utils.PWGLookaheadStream(m, use_graph=False)
    so = utils.PWGLookaheadStream(old, use_graph=False)
    pos = 0
    for i, n in enumerate(sizes):
        f, zz = frames[:, :, pos:pos + n].transpose(1, 2), z[:, 0, pos * 16:(pos + n) * 16]
        yg, ye, yo = sg.push(f, zz), se.push(f, zz), so.push(f, zz)
        assert torch.equal(yg, ye) and torch.equal(yg, yo), (pos, n)
        assert len(sg._graphs) == (0 if i < 3 else 1 if i < 7 else 2)
        pos += n
    assert set(sg._graphs) == {(2, 80), (3, 80)}
    # capturing does not advance the stream
    before = [[t.clone() for t in half] for half in sg._halves]
    cur, counts = sg._cur, (sg.frames_in, sg.frames_out, sg.samples_out)
    f4 = frames[:, :, pos:pos + 4].transpose(1, 2).contiguous()
    sg._capture(f4, z[:, :, pos * 16:(pos + 4) * 16].contiguous())
    assert sg._cur == cur and counts == (sg.frames_in, sg.frames_out, sg.samples_out)
    for half, keep in zip(sg._halves, before):
        for t, k in zip(half, keep):
            assert torch.equal(t, k)
    # new weights: the graphs are dropped, the next replay uses them
    m.load_state_dict({k: v.to(device) for k, v in synth_for(m, 50, 1.0).items()})
    f, zz = frames[:, :, pos:pos + 2].transpose(1, 2), z[:, 0, pos * 16:(pos + 2) * 16]
    yg, ye, yo = sg.push(f, zz), se.push(f, zz), so.push(f, zz)
    assert torch.equal(yg, ye) and not torch.equal(yg, yo)
    assert set(sg._graphs) == {(2, 80)}
    # the flush after replays equals the flush after eager pushes
    assert torch.equal(sg.flush(), se.flush())


@pytest.mark.parametrize("use_graph", [False, True])
def test_stream_draws_noise_outside_the_graph(use_graph, device):
    m, _ = _model(SMALL, 41, device)
    feats = synth.synth_input("c", (1, 80, 24), seed=9)[0].t().to(device)  # (n, C)
    s = utils.PWGLookaheadStream(m, use_graph=use_graph)
    torch.manual_seed(3)
    drawn = [s.push(feats[i:i + 4]) for i in range(0, 24, 4)]
    kept = [y.clone() for y in drawn]
    s.reset()
    zeros = [s.push(feats[i:i + 4], noise=torch.zeros(4 * 16)) for i in range(0, 24, 4)]
    assert [y.shape[1] for y in drawn] == [0, 62, 64, 64, 64, 64]
    for y, k, zero in zip(drawn[1:], kept[1:], zeros[1:]):
        assert torch.isfinite(y).all()
        assert torch.equal(y, k)  # the caller's tensor is not the graph's static buffer: later pushes left it alone
        assert not torch.equal(y, zero)
    assert not torch.equal(drawn[4], drawn[5])
    pcm = s.push_pcm16(feats[:4], noise=torch.zeros(1, 64))
    assert pcm.dtype == torch.int16 and pcm.shape == (1, 64)
