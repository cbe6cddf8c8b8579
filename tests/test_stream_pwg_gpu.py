"""GPU: stateful streaming of the causal Parallel WaveGAN generator -- the one-launch causal layer on a chunk
(csrc/wavenet_stream.hip), the upsampler stage on a chunk (pwg_stretch_conv_stream) and utils.PWGStream end to end
(DESIGN.md s11.3): parity with float64 / the reference golden / the whole-utterance forward, and bit identity across
partitions, batch and graph replay."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import torch_cpu
from parallelwavegan_amd import models, ops, utils
from parallelwavegan_amd.layers.residual_block import WaveNetResidualBlock
from tests.golden import synth
from tests.util import WAVE_TOL, load_golden, max_abs, poison_lds, synth_for

pytestmark = pytest.mark.gpu

DILATIONS = (1, 4, 512)
B, T = 2, 1200
PARTITIONS = ((1, 63, 64, 65, 7, 1000), (1200,), (3,) * 400)
SKIP_SCALE = 0.5


def _rel(a, b):
    """The relative-to-max measure of tests/test_wavenet_layer_gpu.py."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-12)


# ---- the layer ---------------------------------------------------------------------------------------------------------
_LAYER = {}


def _effective_weight(cv):
    """w = g * v / ||v|| per output row, in float64 on the CPU."""
    v, g = cv.weight_v.detach().double(), cv.weight_g.detach().double()
    return v * (g / v.reshape(v.shape[0], -1).norm(dim=1).reshape(-1, 1, 1))


def _layer_case(d):
    """Seeded block (weight-normed, non-zero biases), inputs and the float64 evaluation of the block's formula
    (layers/residual_block.py:102-140 with the causal trim of :118-119), computed once per dilation on the CPU."""
    if d not in _LAYER:
        torch.manual_seed(1000 + d)
        blk = WaveNetResidualBlock(dilation=d, use_causal_conv=True)
        for cv in blk.fused_convs():
            cv.apply_weight_norm()
        with torch.no_grad():
            for p in blk.parameters():
                p.add_(0.1 * torch.randn_like(p))
        g = torch.Generator().manual_seed(d)
        x, c, skips = (torch.randn(B, ch, T, generator=g) for ch in (64, 80, 64))
        w_d, w_a, w_s, w_o = (_effective_weight(cv) for cv in blk.fused_convs())
        b_d, b_s, b_o = (cv.bias.detach().double() for cv in (blk.conv, blk.conv1x1_skip, blk.conv1x1_out))
        xd = x.double()
        z = F.conv1d(F.pad(xd, (2 * d, 0)), w_d, b_d, dilation=d) + F.conv1d(c.double(), w_a)
        gt = torch.tanh(z[:, :64]) * torch.sigmoid(z[:, 64:])
        s_ref = (F.conv1d(gt, w_s, b_s) + skips.double()) * SKIP_SCALE
        x_ref = (F.conv1d(gt, w_o, b_o) + xd) * math.sqrt(0.5)
        _LAYER[d] = dict(state=blk.state_dict(), x=x, c=c, skips=skips, x_ref=x_ref, s_ref=s_ref)
    return _LAYER[d]


def _block(d, device):
    blk = WaveNetResidualBlock(dilation=d, use_causal_conv=True)
    for cv in blk.fused_convs():
        cv.apply_weight_norm()
    blk.load_state_dict(_layer_case(d)["state"])
    return blk.to(device).eval()


def _stream_layer(blk, x, c, skips, parts, check_hist=False, alias=False):
    """Stream (x, c, skips) through ``blk`` in pieces -> (x_out, skips_out).  Both history buffers start as NaN, so a
    start-of-stream read of ``hist_in`` (or an unwritten part of ``hist_out``) shows in the output."""
    nb = x.shape[0]
    hist = [torch.full(blk.history_shape(nb), float("nan"), device=x.device) for _ in range(2)]
    H = hist[0].shape[-1]
    want = torch.zeros_like(hist[0])  # what the history must hold: zeros before the stream
    xs, ss, pos, cur = [], [], 0, 0
    for i, n in enumerate(parts):
        xp, cp = x[:, :, pos:pos + n].contiguous(), c[:, :, pos:pos + n].contiguous()
        sp = None if skips is None else skips[:, :, pos:pos + n].contiguous()
        xo, so = blk.stream_forward(xp, cp, None if i == 0 else hist[cur], hist[1 - cur], skips=sp, skip_scale=SKIP_SCALE,
                                    inplace_skips=alias)
        if alias and sp is not None:
            assert so.data_ptr() == sp.data_ptr()
        cur = 1 - cur
        if check_hist:
            want = torch.cat([want, xp], -1)[..., -H:]
            assert torch.equal(hist[cur], want), (i, n)
        xs.append(xo)
        ss.append(so)
        pos += n
    assert pos == x.shape[-1]
    return torch.cat(xs, -1), torch.cat(ss, -1)


_STREAMED = {}


def _streamed(d, device):
    """Every partition of the layer case streamed once (history checked after every piece), shared by the tests."""
    if d not in _STREAMED:
        case, blk = _layer_case(d), _block(d, device)
        x, c, skips = (case[k].to(device) for k in ("x", "c", "skips"))
        _STREAMED[d] = [_stream_layer(blk, x, c, skips, parts, check_hist=True) for parts in PARTITIONS]
    return _STREAMED[d]


@pytest.mark.parametrize("d", DILATIONS)
def test_layer_matches_float64_oracle(d, device):
    """Figures on an MI355X (relative to max, bound 3e-5): see DESIGN.md s11.3."""
    case = _layer_case(d)
    for parts, (xo, so) in zip(PARTITIONS, _streamed(d, device)):
        for name, got, want in (("x", xo, case["x_ref"]), ("skips", so, case["s_ref"])):
            assert torch.isfinite(got).all(), (name, parts[:3])
            r = _rel(got, want)
            print(f"d={d} pieces={len(parts)} {name}: rel {r:.3e}")
            assert r <= 3e-5, (name, parts[:3], r)


@pytest.mark.parametrize("d", DILATIONS)
def test_layer_under_poisoned_lds(d, device):
    case, blk = _layer_case(d), _block(d, device)
    x, c, skips = (case[k].to(device) for k in ("x", "c", "skips"))
    with poison_lds():
        xo, so = _stream_layer(blk, x, c, skips, PARTITIONS[0])
    ref_x, ref_s = _streamed(d, device)[0]
    assert torch.equal(xo, ref_x) and torch.equal(so, ref_s)
    assert _rel(xo, case["x_ref"]) <= 3e-5 and _rel(so, case["s_ref"]) <= 3e-5


@pytest.mark.parametrize("d", DILATIONS)
def test_layer_partitions_and_batch_are_bit_identical(d, device):
    case, blk = _layer_case(d), _block(d, device)
    outs = _streamed(d, device)  # (also: hist_out after every piece == last H columns of concat(history, piece))
    for xo, so in outs[1:]:
        assert torch.equal(xo, outs[0][0]) and torch.equal(so, outs[0][1])
    x, c, skips = (case[k].to(device) for k in ("x", "c", "skips"))
    for b in range(B):  # lock step == single streams
        xo, so = _stream_layer(blk, x[b:b + 1], c[b:b + 1], skips[b:b + 1], PARTITIONS[0])
        assert torch.equal(xo, outs[0][0][b:b + 1]) and torch.equal(so, outs[0][1][b:b + 1])


def test_layer_skips_aliasing_and_distinct_history(device):
    d = 4
    case, blk = _layer_case(d), _block(d, device)
    x, c, skips = (case[k].to(device) for k in ("x", "c", "skips"))
    ref_x, ref_s = _streamed(d, device)[0]
    # skips_out aliasing skips: the same bits as a separate buffer
    xo, so = _stream_layer(blk, x, c, skips.clone(), PARTITIONS[0], alias=True)
    assert torch.equal(xo, ref_x) and torch.equal(so, ref_s)
    # skips=None == skips=zeros numerically
    x0, s0 = _stream_layer(blk, x, c, None, PARTITIONS[0])
    xz, sz = _stream_layer(blk, x, c, torch.zeros_like(skips), PARTITIONS[0])
    assert torch.equal(x0, xz) and (s0 - sz).abs().max().item() <= 1e-6
    h = torch.zeros(blk.history_shape(B), device=device)
    with pytest.raises(RuntimeError, match="distinct"):
        blk.stream_forward(x[:, :, :8].contiguous(), c[:, :, :8].contiguous(), h, h)


# ---- the upsampler stage -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [4, 3])
@pytest.mark.parametrize("act", [None, "leaky_relu"])
def test_stretch_conv_stream(scale, act, device):
    Tm = 37
    g = torch.Generator().manual_seed(scale)
    x = torch.randn(2, 80, Tm, generator=g)
    w = torch.randn(1, 1, 1, 2 * scale + 1, generator=g) / (2 * scale + 1)
    ref = F.interpolate(x.unsqueeze(1), scale_factor=(1, scale), mode="nearest")
    ref = F.conv2d(ref, w, padding=(0, 2 * scale))[..., :Tm * scale].squeeze(1)
    if act is not None:
        ref = F.leaky_relu(ref, 0.2)
    xd, wd = x.to(device), w.to(device)
    outs = []
    for parts in ((1, 1, 5, 30), (Tm,), (1,) * Tm):
        hist = [torch.full((2, 80, 2), float("nan"), device=device) for _ in range(2)]
        want = torch.zeros(2, 80, 2, device=device)
        ys, pos, cur = [], 0, 0
        for i, n in enumerate(parts):
            xp = xd[:, :, pos:pos + n].contiguous()
            ys.append(ops.stretch_conv_stream(xp, None if i == 0 else hist[cur], hist[1 - cur], wd, scale, 1, act, 0.2))
            cur = 1 - cur
            want = torch.cat([want, xp], -1)[..., -2:]
            assert torch.equal(hist[cur], want), (parts[:2], i)  # the last 2 input columns
            pos += n
        outs.append(torch.cat(ys, -1))
        assert max_abs(outs[-1], ref) <= 3e-5
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    h = torch.zeros(2, 80, 2, device=device)
    with pytest.raises(RuntimeError, match="distinct"):
        ops.stretch_conv_stream(xd, h, h, wd, scale)
    with pytest.raises(RuntimeError, match="freq_kernel"):
        ops.stretch_conv_stream(xd, None, h, torch.zeros(3 * (2 * scale + 1), device=device), scale, freq_kernel=3)


# ---- the generator -----------------------------------------------------------------------------------------------------
def _golden_model(device):
    """Model, noise and mel exactly as tests/test_causal_gpu.py builds them for gold["pwg"]."""
    gold = load_golden("causal_variants")
    seed = int(gold["meta"][0])
    m = models.ParallelWaveGANGenerator(**synth.PWG_CAUSAL)
    sd = synth_for(m, seed + 2, 1.0)
    m.load_state_dict(sd)
    z = synth.synth_input("z", (2, 1, 18 * 16), seed=seed + 2)
    c = synth.synth_input("c", (2, 80, 18 + 4), seed=seed + 2)
    return m.to(device).eval(), sd, z, c, gold["pwg"], seed


def _push_all(stream, frames, noise, parts):
    """frames (B, C, n) and noise (B, 1, n * up) through ``stream`` in pieces -> (B, n * up)."""
    up, ys, pos = stream.up, [], 0
    for n in parts:
        ys.append(stream.push(frames[:, :, pos:pos + n].transpose(1, 2), noise[:, 0, pos * up:(pos + n) * up]))
        assert ys[-1].shape == (frames.shape[0], n * up)
        pos += n
    assert pos == frames.shape[-1]
    return torch.cat(ys, -1)


@pytest.mark.parametrize("use_graph", [False, True])
def test_stream_with_context_matches_reference_golden(use_graph, device):
    m, _, z, c, gold, _ = _golden_model(device)
    with utils.PWGStream(m, batch=2, use_graph=use_graph) as s:
        s.reset(context=c[:, :, :2].transpose(1, 2))
        y = _push_all(s, c[:, :, 2:20].to(device), z.to(device), (1, 7, 2, 8))
        assert (s.frames_in, s.frames_out, s.samples_out) == (18, 18, 288)
        assert s.state_bytes == 2 * 4 * 2 * (3 * 80 * 2 + 64 * 2 * (1 + 2 + 4) * 2)
    err = max_abs(y.unsqueeze(1), gold)
    print(f"graph={use_graph}: max abs vs reference golden {err:.3e}")
    assert err <= WAVE_TOL


def test_stream_replicate_start_matches_oracle_and_inference(device):
    m, sd, z, c, _, _ = _golden_model(device)
    frames = c[:, :, 2:20]
    want = torch_cpu.pwg_generator_causal(sd, z, F.pad(frames, (2, 2), mode="replicate"), **synth.PWG_CAUSAL)
    s = utils.PWGStream(m, batch=2, use_graph=False)
    y = _push_all(s, frames.to(device), z.to(device), (1, 7, 2, 8))
    assert max_abs(y.unsqueeze(1), want) <= WAVE_TOL
    with torch.no_grad():
        for b in range(2):
            own = m.inference(frames[b].t().to(device), x=z[b].t().to(device))  # (T, 1)
            assert max_abs(y[b], own[:, 0]) <= WAVE_TOL
    # a context of the replicated first frame is the same start
    s.reset(context=frames[:, :, :1].expand(-1, -1, 2).transpose(1, 2))
    assert torch.equal(_push_all(s, frames.to(device), z.to(device), (18,)), y)


def test_stream_deep_dilations_end_to_end(device):
    m = models.ParallelWaveGANGenerator(layers=10, stacks=1, use_causal_conv=True,
                                        upsample_params={"upsample_scales": [4, 4]})
    m.load_state_dict(synth_for(m, 77, 1.0))
    m = m.to(device).eval()
    n, up = 80, 16
    frames = synth.synth_input("c", (2, 80, n), seed=77).to(device)
    z = synth.synth_input("z", (2, 1, n * up), seed=77).to(device)
    s = utils.PWGStream(m, batch=2, use_graph=False)
    assert s.state_bytes == 2 * 4 * 2 * (3 * 80 * 2 + 64 * 2 * 1023)
    outs = []
    for parts in ((1,) * n, (n,), (3, 1, 17, 59)):
        s.reset()
        outs.append(_push_all(s, frames, z, parts))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    s.reset()
    assert torch.equal(_push_all(s, frames, z, (3, 1, 17, 59)), outs[0])  # reset() and a second pass
    single = utils.PWGStream(m, batch=1, use_graph=False)
    for b in range(2):
        single.reset()
        assert torch.equal(_push_all(single, frames[b:b + 1], z[b:b + 1], (3, 1, 17, 59)), outs[0][b:b + 1])
    with torch.no_grad():
        whole = m(z, F.pad(frames, (2, 2), mode="replicate"))
    err = max_abs(outs[0].unsqueeze(1), whole)
    print(f"deep dilations: max abs vs the whole-utterance forward {err:.3e}")
    assert torch.isfinite(outs[0]).all() and err <= WAVE_TOL


def test_stream_graph_replay_is_bit_identical_to_eager(device):
    m, _, _, _, _, seed = _golden_model(device)
    sizes = (2, 2, 2, 2, 2, 2, 3, 2)  # eager start, then A -> B -> A ... over 5 replays of one size, another size, back
    total = sum(sizes)
    frames = synth.synth_input("c", (1, 80, total + 4), seed=5).to(device)
    z = synth.synth_input("z", (1, 1, (total + 4) * 16), seed=5).to(device)
    old = copy.deepcopy(m)
    sg, se = utils.PWGStream(m, use_graph=True), utils.PWGStream(m, use_graph=False)
    so = utils.PWGStream(old, use_graph=False)
    pos = 0
    for n in sizes:
        f, zz = frames[:, :, pos:pos + n].transpose(1, 2), z[:, 0, pos * 16:(pos + n) * 16]
        yg, ye, yo = sg.push(f, zz), se.push(f, zz), so.push(f, zz)
        assert torch.equal(yg, ye) and torch.equal(yg, yo), (pos, n)
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
    m.load_state_dict({k: v.to(device) for k, v in synth_for(m, seed + 9, 1.0).items()})
    f, zz = frames[:, :, pos:pos + 2].transpose(1, 2), z[:, 0, pos * 16:(pos + 2) * 16]
    yg, ye, yo = sg.push(f, zz), se.push(f, zz), so.push(f, zz)
    assert torch.equal(yg, ye) and not torch.equal(yg, yo)
    assert set(sg._graphs) == {(2, 80)}


@pytest.mark.parametrize("use_graph", [False, True])
def test_stream_draws_noise_outside_the_graph(use_graph, device):
    m, _, _, c, _, _ = _golden_model(device)
    feats = c[0, :, :12].t().to(device)  # (n, C)
    s = utils.PWGStream(m, use_graph=use_graph)
    torch.manual_seed(3)
    drawn = [s.push(feats[i:i + 4]) for i in (0, 4, 8)]
    kept = [y.clone() for y in drawn]
    s.reset()
    zeros = [s.push(feats[i:i + 4], noise=torch.zeros(4 * 16)) for i in (0, 4, 8)]
    for y, k, zero in zip(drawn, kept, zeros):
        assert y.shape == (1, 64) and torch.isfinite(y).all()
        assert torch.equal(y, k)  # the caller's tensor is not the graph's static buffer: later pushes left it alone
        assert not torch.equal(y, zero)
    assert not torch.equal(drawn[1], drawn[2])
    pcm = s.push_pcm16(feats[:4], noise=torch.zeros(1, 64))
    assert pcm.dtype == torch.int16 and pcm.shape == (1, 64)
