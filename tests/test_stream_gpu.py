"""GPU: stateful streaming synthesis (csrc/conv1d_stream.hip, utils.CausalStream) -- the streamed layers against the
oracle, the streamed causal generators against the reference's goldens and against the package's own whole-utterance
forward, bit-identical audio for every partition of the same frames, and the state handling around it."""
import pytest
import torch

from oracle import torch_cpu
from parallelwavegan_amd import layers, models
from parallelwavegan_amd.utils import CausalStream, streaming
from tests.golden import synth
from tests.util import WAVE_TOL, load_golden, max_abs, poison_lds, synth_for

pytestmark = pytest.mark.gpu

HIFIGAN_V1_CAUSAL = dict(synth.HIFIGAN_V1, use_causal_conv=True)


def _load(cls, cfg, seed, g_scale, device):
    m = cls(**cfg)
    m.load_state_dict(synth_for(m, seed, g_scale))
    return m.to(device).eval()


def _stream_layer(layer, x, pieces, **fused):
    """Feed x (B, C, T) through ``layer.stream_forward`` in ``pieces`` with ping-pong history; concatenated result."""
    assert sum(pieces) == x.shape[-1]
    hist = [torch.full(layer.history_shape(x.shape[0]), float("nan"), device=x.device) for _ in range(2)]
    outs, t, cur = [], 0, None
    for n in pieces:
        nxt = 0 if cur is None else 1 - cur
        outs.append(layer.stream_forward(x[..., t:t + n].contiguous(), None if cur is None else hist[cur], hist[nxt],
                                         **fused))
        cur, t = nxt, t + n
    return torch.cat(outs, -1)


def _stream(model, c, pieces, **kw):
    """Push c (B, C, T) through a CausalStream in ``pieces`` frames at a time -> (B, T * upsample_factor)."""
    assert sum(pieces) == c.shape[-1]
    s = kw.pop("stream", None) or CausalStream(model, batch=c.shape[0], **kw)
    feats = c.transpose(1, 2).contiguous()
    outs, t = [], 0
    for n in pieces:
        outs.append(s.push(feats[:, t:t + n]))
        t += n
    s.close()
    assert s.frames_in == s.frames_out == c.shape[-1]
    return torch.cat(outs, -1)


# ---- 1. layers against the oracle --------------------------------------------------------------------------------
def test_streamed_layers_match_oracle(device):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 24, 50, generator=g)
    conv = layers.CausalConv1d(24, 40, 5, dilation=3)
    w, b = conv.conv.weight.detach().clone(), conv.conv.bias.detach().clone()
    y_ref = torch_cpu.causal_conv1d(torch.nn.functional.leaky_relu(x, 0.1), w, b, 3)
    conv = conv.to(device)
    for pieces in ((1, 7, 2, 13, 5, 1, 21), (50,), (1,) * 50):
        y = _stream_layer(conv, x.to(device), pieces, pre_act="leaky_relu", pre_slope=0.1)
        err = max_abs(y, y_ref)
        print("causal conv", pieces[:4], err)
        assert err < 3e-5

    x = torch.randn(2, 24, 30, generator=g)
    up = layers.CausalConvTranspose1d(24, 12, 8, 4)
    w, b = up.deconv.weight.detach().clone(), up.deconv.bias.detach().clone()
    y_ref = torch_cpu.causal_conv_transpose1d(x, w, b, 4)
    up = up.to(device)
    for pieces in ((1, 7, 2, 13, 7), (30,), (1,) * 30):
        y = _stream_layer(up, x.to(device), pieces)
        assert y.shape[-1] == 30 * 4
        err = max_abs(y, y_ref)
        print("causal transposed conv", pieces[:4], err)
        assert err < 3e-5


@pytest.mark.parametrize("pad,mode", [("ReflectionPad1d", "reflect"), ("ReplicationPad1d", "replicate")])
def test_streamed_layer_start_of_stream_padding(pad, mode, device):
    """Reflect / replicate start-of-stream context against torch.nn.functional.pad + conv on the CPU; the fused
    pre-activation, bias, an addend, out_mul and tanh ride along."""
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 24, 50, generator=g)
    add = torch.randn(2, 40, 50, generator=g)
    conv = layers.CausalConv1d(24, 40, 5, dilation=3, pad=pad, pad_params={})
    w, b = conv.conv.weight.detach().clone(), conv.conv.bias.detach().clone()
    xp = torch.nn.functional.pad(torch.nn.functional.leaky_relu(x, 0.2), (12, 0), mode=mode)
    y_ref = torch.tanh((torch.nn.functional.conv1d(xp, w, b, dilation=3) + add) * 0.5)
    conv = conv.to(device)
    for pieces in ((14, 1, 7, 2, 13, 13), (50,), (13,) + (1,) * 37):  # reflect mirrors 12 columns: first piece >= 13
        hist = [torch.full(conv.history_shape(2), float("nan"), device=device) for _ in range(2)]
        outs, t, cur = [], 0, None
        for n in pieces:
            nxt = 0 if cur is None else 1 - cur
            outs.append(conv.stream_forward(x[..., t:t + n].contiguous().to(device), None if cur is None else hist[cur],
                                            hist[nxt], pre_act="leaky_relu", pre_slope=0.2,
                                            add1=add[..., t:t + n].contiguous().to(device), out_mul=0.5, post_act="tanh"))
            cur, t = nxt, t + n
        err = max_abs(torch.cat(outs, -1), y_ref)
        print(mode, pieces[:4], err)
        assert err < 3e-5
    if mode == "reflect":  # too short a first piece cannot be mirrored: an error, not garbage
        with pytest.raises(RuntimeError, match="reflect"):
            conv.stream_forward(x[..., :12].contiguous().to(device), None, torch.empty(conv.history_shape(2), device=device))


def test_history_buffers_must_be_distinct(device):
    conv = layers.CausalConv1d(8, 8, 3).to(device)
    h = torch.zeros(conv.history_shape(1), device=device)
    with pytest.raises(RuntimeError, match="distinct"):
        conv.stream_forward(torch.zeros(1, 8, 4, device=device), h, h)


# ---- 2. reference goldens ----------------------------------------------------------------------------------------
def test_streamed_generators_match_reference_golden(device):
    gold = load_golden("causal_variants")
    seed = int(gold["meta"][0])
    g = _load(models.HiFiGANGenerator, synth.HIFIGAN_CAUSAL, seed, float(gold["g_scale"]), device)
    c = synth.synth_input("c", (2, 80, 24), seed=seed).to(device)
    for kw in (dict(use_graph=False), dict(use_graph=True)):
        y = _stream(g, c, (1, 7, 2, 13, 1), **kw)
        err = max_abs(y.unsqueeze(1), gold["hifigan"])
        print("hifigan", kw, err)
        assert err <= WAVE_TOL
    m = _load(models.MelGANGenerator, synth.MELGAN_CAUSAL, seed + 1, synth.MELGAN_G_SCALE, device)
    c = synth.synth_input("c", (2, 80, 20), seed=seed + 1).to(device)
    for kw in (dict(use_graph=False), dict(use_graph=True)):
        y = _stream(m, c, (3, 5, 1, 7, 4), **kw)  # 3 < warmup_frames = 7: held, emitted with the second push
        err = max_abs(y.unsqueeze(1), gold["melgan"])
        print("melgan", kw, err)
        assert err <= WAVE_TOL


# ---- 3. against the package's own whole-utterance forward ----------------------------------------------------------
def _v1_causal(device):
    g = models.HiFiGANGenerator(**HIFIGAN_V1_CAUSAL)
    g.load_state_dict(synth_for(g, 11, 1.25))
    g.remove_weight_norm()
    return g.to(device).eval()


@pytest.mark.parametrize("family", ["hifigan_causal", "melgan_causal", "hifigan_v1_causal"])
def test_streamed_equals_whole_utterance_forward(family, device):
    if family == "hifigan_v1_causal":
        model = _v1_causal(device)
    elif family == "hifigan_causal":
        model = _load(models.HiFiGANGenerator, synth.HIFIGAN_CAUSAL, 3, 1.0, device)
    else:
        model = _load(models.MelGANGenerator, synth.MELGAN_CAUSAL, 4, synth.MELGAN_G_SCALE, device)
    frames = 216
    c = torch.randn(2, 80, frames, generator=torch.Generator().manual_seed(8)).to(device)
    with torch.no_grad():
        full = model(c)[:, 0]
    for pieces in ((8,) * 27, (40, 1, 7, 2, 13, 33, 64, 56)):
        y = _stream(model, c, pieces)
        err = max_abs(y, full)
        print(family, pieces[:3], err)
        assert err <= 2e-5


# ---- 4. / 7. partition invariance, bit for bit (also with poisoned LDS) -------------------------------------------
def _partitions(frames, warm):
    return [(frames,), (warm,) + (1,) * (frames - warm), (warm, 1, 5, 1, 17, 3, frames - warm - 27),
            (warm + 2, 9, 1, 1, 30, frames - warm - 43)]


def _check_partition_invariance(device):
    for cls, cfg, seed, scale in ((models.HiFiGANGenerator, synth.HIFIGAN_CAUSAL, 3, 1.0),
                                  (models.MelGANGenerator, synth.MELGAN_CAUSAL, 4, synth.MELGAN_G_SCALE)):
        model = _load(cls, cfg, seed, scale, device)
        warm = CausalStream.required_warmup_frames(model)
        frames = 72
        c = torch.randn(2, 80, frames, generator=torch.Generator().manual_seed(9)).to(device)
        outs = [_stream(model, c, p, use_graph=False) for p in _partitions(frames, warm)]
        assert torch.isfinite(outs[0]).all() and outs[0].abs().max() > 1e-3
        for p, y in zip(_partitions(frames, warm)[1:], outs[1:]):
            assert torch.equal(y, outs[0]), (cls.__name__, p[:4], max_abs(y, outs[0]))
        # graph replay: the same bits as eager, for a regular and an irregular partition
        fives = (warm,) + (5,) * ((frames - warm) // 5)
        fives += (frames - sum(fives),) if sum(fives) < frames else ()
        for p in (fives, _partitions(frames, warm)[2]):
            assert torch.equal(_stream(model, c, p, use_graph=True), outs[0]), (cls.__name__, "graph", p[:4])


def test_partition_invariance_bit_for_bit(device):
    _check_partition_invariance(device)


def test_partition_invariance_with_poisoned_lds(device):
    with poison_lds():
        _check_partition_invariance(device)


def test_v1_geometry_partition_invariance(device):
    """All four tile shapes of the stream kernel meet at the V1 geometry (8 .. 2048+ columns per push)."""
    model = _v1_causal(device)
    c = torch.randn(1, 80, 48, generator=torch.Generator().manual_seed(10)).to(device)
    ref = _stream(model, c, (48,), use_graph=False)
    for p in ((8,) * 6, (1, 2, 4, 8, 33), (1,) * 48):
        assert torch.equal(_stream(model, c, p, use_graph=False), ref), p[:4]
    assert torch.equal(_stream(model, c, (8,) * 6, use_graph=True), ref)


# MelGAN at the recipe's widths: 256 and 128 channels behind the k = 16 / k = 4 upsampling layers, 8 and 16 columns per
# frame.  At these widths the general convolution kernel has several tiles and reduction splits to choose from, by
# column count and batch -- the 1 x 1 layers of a ResidualStack must not inherit that choice in a stream.
# These are also the tests that reach the stream kernel's 32 x 64 tile in fp32: one push of 208 frames at batch 3 is
# 1664 columns at 256 rows, 8 x 26 x 3 = 624 workgroups of 32 rows (the dispatch rule wants 512), and the batched test
# compares it bit for bit with the batch-1 streams (208 workgroups: the 16-row tile).  So no separate fp32 case exists;
# the bf16 kernel's is tests/test_stream_bf16_gpu.py::test_streamed_bf16_conv_32_row_tile.
MELGAN_WIDE_CAUSAL = dict(in_channels=80, out_channels=1, kernel_size=7, channels=512, upsample_scales=[8, 2],
                          stack_kernel_size=3, stacks=2, use_causal_conv=True)


@pytest.fixture(scope="module")
def melgan_wide(device):
    model = _load(models.MelGANGenerator, MELGAN_WIDE_CAUSAL, 21, synth.MELGAN_G_SCALE, device)
    frames = 208  # one push: 1664 / 3328 columns in the two stages; frame by frame: 8 / 16
    c = torch.randn(3, 80, frames, generator=torch.Generator().manual_seed(22)).to(device)
    whole = [_stream(model, c[i:i + 1], (frames,), use_graph=False) for i in range(3)]
    return model, c, whole


def test_melgan_recipe_width_partition_invariance_batch_1(melgan_wide):
    model, c, whole = melgan_wide
    frames, warm = c.shape[-1], CausalStream.required_warmup_frames(model)
    assert warm == 7
    with torch.no_grad():
        assert max_abs(whole[0], model(c[:1])[:, 0]) <= 2e-5
    assert whole[0].abs().max() > 1e-3
    for p in ((8,) * 26, (warm,) + (1,) * (frames - warm), (36, 100, 1, 5, 66), (warm, 1, 200)):
        y = _stream(model, c[:1], p, use_graph=False)
        assert torch.equal(y, whole[0]), (p[:4], max_abs(y, whole[0]))
    assert torch.equal(_stream(model, c[:1], (8,) * 26, use_graph=True), whole[0])


def test_melgan_recipe_width_batched_streams_equal_single_streams(melgan_wide):
    model, c, whole = melgan_wide
    frames = c.shape[-1]
    for p in ((frames,), (8,) * 26, (36, 100, 1, 5, 66)):
        together = _stream(model, c, p, use_graph=False)
        for i in range(3):
            assert torch.equal(together[i], whole[i][0]), (p[:4], i, max_abs(together[i], whole[i][0]))


def test_melgan_partition_invariance_batch_1(device):
    """The default ``CausalStream(batch=1)`` on the golden MelGAN config, eager and graph replay."""
    model = _load(models.MelGANGenerator, synth.MELGAN_CAUSAL, 4, synth.MELGAN_G_SCALE, device)
    warm, frames = CausalStream.required_warmup_frames(model), 72
    c = torch.randn(1, 80, frames, generator=torch.Generator().manual_seed(23)).to(device)
    parts = _partitions(frames, warm)
    ref = _stream(model, c, parts[0], use_graph=False)
    for p in parts[1:]:
        assert torch.equal(_stream(model, c, p, use_graph=False), ref), p[:4]
    for p in (parts[2], (warm,) + (5,) * 13):
        assert torch.equal(_stream(model, c, p, use_graph=True), ref), ("graph", p[:4])


def test_graph_cache_is_bounded(device):
    """Only ``max_graph_shapes`` chunk sizes keep their graphs; an evicted size is captured again and gives the same bits."""
    model = _load(models.HiFiGANGenerator, synth.HIFIGAN_CAUSAL, 3, 1.0, device)
    c = torch.randn(1, 80, 42, generator=torch.Generator().manual_seed(24)).to(device)
    pieces = (1, 2, 3, 4, 5, 6, 2, 7, 1, 5, 6)  # seven sizes; the first push of a stream is eager
    ref = _stream(model, c, pieces, use_graph=False)
    s = CausalStream(model, use_graph=True)
    assert torch.equal(_stream(model, c, pieces, stream=s), ref)
    assert len(s._graphs) == CausalStream.max_graph_shapes == 4
    assert [k[0] for k in s._graphs] == [7, 1, 5, 6]


# ---- 5. the comparison can fail -----------------------------------------------------------------------------------
def test_forgotten_reset_shows_up(device):
    model = _load(models.HiFiGANGenerator, synth.HIFIGAN_CAUSAL, 3, 1.0, device)
    gen = torch.Generator().manual_seed(12)
    c1, c2 = (torch.randn(1, 80, 40, generator=gen).to(device) for _ in range(2))
    with torch.no_grad():
        full2 = model(c2)[:, 0]
    s = CausalStream(model, use_graph=False)
    _stream(model, c1, (8,) * 5, stream=s)
    s.frames_in = s.frames_out = 0
    carried = _stream(model, c2, (8,) * 5, stream=s)  # state of utterance 1 carried into utterance 2
    up = model.upsample_factor
    assert max_abs(carried[:, :4 * up], full2[:, :4 * up]) > 1e-3
    s.reset()
    assert max_abs(_stream(model, c2, (8,) * 5, stream=s), full2) <= 2e-5


# ---- 6. state -----------------------------------------------------------------------------------------------------
def test_reset_restores_start_of_stream(device):
    for cls, cfg, seed, scale in ((models.HiFiGANGenerator, synth.HIFIGAN_CAUSAL, 3, 1.0),
                                  (models.MelGANGenerator, synth.MELGAN_CAUSAL, 4, synth.MELGAN_G_SCALE)):
        model = _load(cls, cfg, seed, scale, device)
        c = torch.randn(1, 80, 32, generator=torch.Generator().manual_seed(13)).to(device)
        s = CausalStream(model)
        first = _stream(model, c, (8,) * 4, stream=s)
        assert s.state_bytes == 2 * 4 * sum(torch.Size(l.history_shape(1)).numel() for l, _ in model.stream_layers())
        s.reset()
        assert s.frames_in == s.frames_out == 0
        assert torch.equal(_stream(model, c, (8,) * 4, stream=s), first)


def test_batched_streams_equal_single_streams(device):
    model = _load(models.HiFiGANGenerator, synth.HIFIGAN_CAUSAL, 3, 1.0, device)
    c = torch.randn(3, 80, 40, generator=torch.Generator().manual_seed(14)).to(device)
    together = _stream(model, c, (8, 1, 7, 24))
    for i in range(3):
        alone = _stream(model, c[i:i + 1], (8, 1, 7, 24))
        assert torch.equal(alone[0], together[i]), i
    # (n, C) features are the batch-1 form
    s = CausalStream(model)
    assert torch.equal(s.push(c[0].t().contiguous()), _stream(model, c[:1], (40,)))


def test_new_weights_are_never_replayed_from_an_old_graph(device):
    model = _load(models.HiFiGANGenerator, synth.HIFIGAN_CAUSAL, 3, 1.0, device)
    c = torch.randn(1, 80, 40, generator=torch.Generator().manual_seed(15)).to(device)
    s = CausalStream(model, use_graph=True)
    old = _stream(model, c, (8,) * 5, stream=s)
    other = models.HiFiGANGenerator(**synth.HIFIGAN_CAUSAL)
    model.load_state_dict(synth_for(other, 77, 1.1))
    s.reset()
    new = _stream(model, c, (8,) * 5, stream=s)
    with torch.no_grad():
        full = model(c)[:, 0]
    assert max_abs(new, full) <= 2e-5
    assert max_abs(new, old) > 1e-3
    model.remove_weight_norm()  # changes the parameter set between pushes of one chunk size as well
    s.reset()
    assert max_abs(_stream(model, c, (8,) * 5, stream=s), full) <= 2e-5


def test_normalize_before_and_pcm16(device):
    model = _load(models.HiFiGANGenerator, synth.HIFIGAN_CAUSAL, 3, 1.0, device)
    gen = torch.Generator().manual_seed(16)
    mean, scale = torch.randn(80, generator=gen), torch.rand(80, generator=gen) + 0.5
    with pytest.raises(ValueError, match="register_stats"):
        CausalStream(model, normalize_before=True)
    model.register_buffer("mean", mean.to(device))
    model.register_buffer("scale", scale.to(device))
    f = (torch.randn(40, 80, generator=gen) * scale + mean).to(device)
    full = model.inference(f, normalize_before=True).reshape(-1)
    s = CausalStream(model, normalize_before=True)
    y = torch.cat([s.push(f[t:t + 8]) for t in range(0, 40, 8)], -1)
    assert max_abs(y[0], full) <= 2e-5
    s.reset()
    pcm = torch.cat([s.push_pcm16(f[t:t + 8]) for t in range(0, 40, 8)], -1)
    assert pcm.dtype == torch.int16 and torch.equal(pcm, streaming.to_pcm16(y))


def test_short_utterance_on_a_reflect_padded_model_raises(device):
    model = _load(models.MelGANGenerator, synth.MELGAN_CAUSAL, 4, synth.MELGAN_G_SCALE, device)
    c = torch.randn(1, 6, 80, generator=torch.Generator().manual_seed(17)).to(device)
    with pytest.raises(RuntimeError, match="needs 7"):
        with CausalStream(model) as s:
            assert s.warmup_frames == 7
            assert s.push(c[:, :4]).shape == (1, 0) and s.push(c[:, 4:]).shape == (1, 0)
            assert s.frames_in == 6 and s.frames_out == 0
    with pytest.raises(ValueError, match="expected"):
        CausalStream(model, batch=2).push(c)
