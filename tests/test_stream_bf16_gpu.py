"""GPU: streaming with bf16 operands (csrc/conv1d_stream_bf16.hip, ``CausalStream(model, precision="bf16")``).

Layers: inputs and weights are drawn and rounded to bf16-representable fp32 values BEFORE the call (with a pre-activation
the ACTIVATED input is what is rounded, as in tests/test_conv_bf16_gpu.py), so the streamed result can differ from the
float64 causal convolution of the same operands only by fp32 accumulation order: the bar is the project's per-layer bar
(RTOL of test_conv_bf16_gpu.py).  The history a bf16 launch writes is raw fp32 and must equal the fp32 launch's bit for
bit.  Generators: any partition of the same frames gives the same bits (the sum order of an output element depends on
the layer alone), and the error against the fp32 oracle is the CPU emulation's error (FACTOR of
tests/test_hifigan_bf16_gpu.py).
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import torch_cpu
from parallelwavegan_amd import layers, models, ops
from parallelwavegan_amd.layers.causal_conv import stream_pointwise
from parallelwavegan_amd.layers.conv import each_conv
from parallelwavegan_amd.utils import CausalStream
from tests.bf16_emulation import bf16_operands, rms
from tests.golden import synth
from tests.test_conv_bf16_gpu import RTOL
from tests.test_hifigan_bf16_gpu import FACTOR
from tests.test_stream_gpu import HIFIGAN_V1_CAUSAL, MELGAN_WIDE_CAUSAL
from tests.test_stream_mb_host import MB_CAUSAL
from tests.util import max_abs, poison_lds, synth_for

pytestmark = pytest.mark.gpu

BF16_STREAM, FP32_STREAM = "conv1d_stream_bf16_kernel", "conv1d_stream_kernel"
OTHER_CONVS = (FP32_STREAM, "conv1d_mfma_dma_kernel", "conv1d_bf16_mfma_kernel")


def _bf16r(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _act(x, kind, slope):
    return F.leaky_relu(x, slope) if kind == "leaky_relu" else x


def _nan(shape, device):
    return torch.full(shape, float("nan"), device=device)


def _stream_layer(layer, x, pieces, add1=None, check_history=True, **fused):
    """x (B, C, T) through ``layer.stream_forward(precision="bf16")`` in ``pieces`` with NaN-filled ping-pong history ->
    concatenated result.  After every launch the history written must equal what the fp32 launch writes for the same
    ``x`` / ``hist_in``."""
    assert sum(pieces) == x.shape[-1]
    up = getattr(layer, "stride", 1)
    hist = [_nan(layer.history_shape(x.shape[0]), x.device) for _ in range(2)]
    outs, t, cur = [], 0, None
    for n in pieces:
        nxt = 0 if cur is None else 1 - cur
        xn = x[..., t:t + n].contiguous()
        kw = dict(fused, add1=add1[..., t * up:(t + n) * up].contiguous()) if add1 is not None else fused
        h_in = None if cur is None else hist[cur]
        outs.append(layer.stream_forward(xn, h_in, hist[nxt], precision="bf16", **kw))
        if check_history:
            h32 = _nan(hist[nxt].shape, x.device)
            layer.stream_forward(xn, h_in, h32, **kw)
            assert torch.equal(hist[nxt], h32), ("history", n, t)
        cur, t = nxt, t + n
    return torch.cat(outs, -1)


def _pieces(T, first=1):
    """One piece; column by column; irregular: pieces shorter than H and the tile boundaries 16 / 17 / 33 / 70."""
    irregular = (first, 16, 17, 33, 70, 2, 1)
    assert sum(irregular) < T
    return [(T,), (first,) + (1,) * (T - first), irregular + (T - sum(irregular),)]


def _rel_err(y, ref):
    y = y.cpu().double()
    assert y.shape == ref.shape and torch.isfinite(y).all()
    return (y - ref).abs().max().item() / (ref.abs().max().item() + 1e-12)


# ---- 1. / 3. layers against float64 of the same rounded operands; history against the fp32 launch ----------------
# (c_in, c_out, k, d, batch, epilogue): c_in 24 / 80: channel padding inside a chunk; 32: one chunk; 64: two; 160: five
# chunks in two staged blocks; 512: four blocks.  c_out 1 / 24 / 40: row padding inside the image and rows no multiple of
# 16; 256: sixteen row blocks.  (3, 27): H = 54, (11, 5): H = 50 -- pieces shorter than H
CONV_CASES = [
    (24, 40, 7, 1, 1, "pre"),
    (32, 1, 3, 27, 3, "tanh"),
    (64, 24, 11, 5, 1, "add_div"),
    (80, 256, 5, 3, 3, "pre"),
    (160, 40, 3, 27, 1, "add_div"),
    (512, 24, 7, 1, 3, "pre"),
    (160, 256, 11, 5, 1, "tanh"),
    (512, 40, 5, 3, 1, None),
]
POINTWISE_CASES = [(512, 256, 3, "add_div"), (160, 1, 1, "pre"), (24, 40, 1, None), (64, 24, 3, "tanh")]
# (c_in, c_out, k, s, batch): c_out * s = 2, 48 and 96 (below 128), 160 and 192 (above)
TRANSPOSED_CASES = [(32, 1, 4, 2, 3, "pre"), (64, 24, 4, 2, 1, "pre"), (80, 40, 8, 4, 3, None), (512, 24, 16, 8, 1, "pre"),
                    (160, 24, 8, 4, 1, "add_div")]
T = 150


def _epilogue(kind, g, shape):
    """-> (fused keywords, add1 or None, reference epilogue)"""
    if kind == "pre":
        return dict(pre_act="leaky_relu", pre_slope=0.1), None, lambda r: r
    if kind == "tanh":
        return dict(pre_act="leaky_relu", pre_slope=0.01, post_act="tanh"), None, torch.tanh
    if kind == "add_div":
        add = torch.randn(shape, generator=g)
        return dict(out_div=3.0), add, lambda r: (r + add.double()) / 3.0
    return {}, None, lambda r: r


def _set(cv, w, b):
    with torch.no_grad():
        cv.weight.copy_(w)
        cv.bias.copy_(b)


@pytest.fixture(scope="module")
def worst():
    errs = {}
    yield errs
    if errs:
        print("worst per-layer rel-to-max error:", max(errs.items(), key=lambda kv: kv[1]))


@pytest.mark.parametrize("c_in,c_out,k,d,batch,epi", CONV_CASES)
def test_streamed_bf16_conv_matches_float64_of_rounded_operands(c_in, c_out, k, d, batch, epi, device, worst):
    g = torch.Generator().manual_seed(c_in * 31 + c_out * 7 + k)
    x = _bf16r(torch.randn(batch, c_in, T, generator=g))
    w = _bf16r(torch.randn(c_out, c_in, k, generator=g) / (c_in * k) ** 0.5)
    b = torch.randn(c_out, generator=g)
    fused, add, post = _epilogue(epi, g, (batch, c_out, T))
    xa = _bf16r(_act(x, fused.get("pre_act"), fused.get("pre_slope", 0.0)))
    ref = post(torch_cpu.causal_conv1d(xa.double(), w.double(), b.double(), d))
    layer = layers.CausalConv1d(c_in, c_out, k, dilation=d)
    _set(layer.conv, w, b)
    layer = layer.to(device)
    for pieces in _pieces(T):
        y = _stream_layer(layer, x.to(device), pieces, None if add is None else add.to(device), **fused)
        err = _rel_err(y, ref)
        print(f"conv {c_in}->{c_out} k{k} d{d} B{batch} {epi} pieces {pieces[:3]}: rel-to-max error {err:.3e}")
        worst[(c_in, c_out, k, d, pieces[:2])] = err
        assert err <= RTOL


def test_streamed_bf16_conv_32_row_tile(device, worst):
    """The 32 x 64 tile, which no other case here reaches: c_out 512, 256 columns, batch 8 is 16 x 4 x 8 = 512
    workgroups of 32 rows, the threshold of the dispatch rule.  Same reference and bar as the cases above; and stream 0
    alone, in four chunks of 64 (16 workgroups: the 16-row tile), gives the same bits -- the tile does not change an
    element's sum order."""
    c_in, c_out, k, n, batch = 32, 512, 3, 256, 8
    g = torch.Generator().manual_seed(c_in * 31 + c_out * 7 + k)
    x = _bf16r(torch.randn(batch, c_in, n, generator=g))
    w = _bf16r(torch.randn(c_out, c_in, k, generator=g) / (c_in * k) ** 0.5)
    b = torch.randn(c_out, generator=g)
    fused, _, post = _epilogue("pre", g, None)
    xa = _bf16r(_act(x, fused["pre_act"], fused["pre_slope"]))
    ref = post(torch_cpu.causal_conv1d(xa.double(), w.double(), b.double(), 1))
    layer = layers.CausalConv1d(c_in, c_out, k)
    _set(layer.conv, w, b)
    layer = layer.to(device)
    y = _stream_layer(layer, x.to(device), (n,), **fused)
    err = _rel_err(y, ref)
    print(f"conv {c_in}->{c_out} k{k} B{batch} one push of {n}: rel-to-max error {err:.3e}")
    worst[(c_in, c_out, k, 1, (n,))] = err
    assert err <= RTOL
    alone = _stream_layer(layer, x[:1].to(device), (64,) * 4, **fused)
    assert torch.equal(alone[0], y[0]), max_abs(alone[0], y[0])


@pytest.mark.parametrize("c_in,c_out,batch,epi", POINTWISE_CASES)
def test_streamed_bf16_pointwise_matches_float64_of_rounded_operands(c_in, c_out, batch, epi, device, worst):
    g = torch.Generator().manual_seed(c_in * 31 + c_out * 7 + 1)
    x = _bf16r(torch.randn(batch, c_in, T, generator=g))
    w = _bf16r(torch.randn(c_out, c_in, 1, generator=g) / c_in ** 0.5)
    b = torch.randn(c_out, generator=g)
    fused, add, post = _epilogue(epi, g, (batch, c_out, T))
    xa = _bf16r(_act(x, fused.get("pre_act"), fused.get("pre_slope", 0.0)))
    ref = post(F.conv1d(xa.double(), w.double(), b.double()))
    cv = layers.Conv1d(c_in, c_out, 1)
    _set(cv, w, b)
    cv = cv.to(device)
    for pieces in _pieces(T):
        outs, t = [], 0
        for n in pieces:
            kw = dict(fused, add1=add[..., t:t + n].contiguous().to(device)) if add is not None else fused
            outs.append(stream_pointwise(cv, x[..., t:t + n].contiguous().to(device), precision="bf16", **kw))
            t += n
        err = _rel_err(torch.cat(outs, -1), ref)
        print(f"1x1 {c_in}->{c_out} B{batch} {epi} pieces {pieces[:3]}: rel-to-max error {err:.3e}")
        worst[(c_in, c_out, 1, 1, pieces[:2])] = err
        assert err <= RTOL


def _transposed_ref(xa, w, b, s, mode):
    xp = F.pad(xa.double(), (1, 0), mode=mode)
    return F.conv_transpose1d(xp, w.double(), b.double(), stride=s)[:, :, s:-s]


@pytest.mark.parametrize("c_in,c_out,k,s,batch,epi", TRANSPOSED_CASES)
def test_streamed_bf16_transposed_conv_matches_float64_of_rounded_operands(c_in, c_out, k, s, batch, epi, device, worst):
    g = torch.Generator().manual_seed(c_in * 31 + c_out * 7 + k)
    x = _bf16r(torch.randn(batch, c_in, T, generator=g))
    w = _bf16r(torch.randn(c_in, c_out, k, generator=g) / (c_in * 2) ** 0.5)
    b = torch.randn(c_out, generator=g)
    fused, add, post = _epilogue(epi, g, (batch, c_out, T * s))
    xa = _bf16r(_act(x, fused.get("pre_act"), fused.get("pre_slope", 0.0)))
    ref = post(_transposed_ref(xa, w, b, s, "replicate"))
    layer = layers.CausalConvTranspose1d(c_in, c_out, k, s)
    _set(layer.deconv, w, b)
    layer = layer.to(device)
    for pieces in _pieces(T):
        y = _stream_layer(layer, x.to(device), pieces, None if add is None else add.to(device), **fused)
        err = _rel_err(y, ref)
        print(f"transposed {c_in}->{c_out} k{k} s{s} B{batch} {epi} pieces {pieces[:3]}: rel-to-max error {err:.3e}")
        worst[(c_in, c_out, k, -s, pieces[:2])] = err
        assert err <= RTOL


# ---- 2. start-of-stream padding -------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad,mode", [("ReflectionPad1d", "reflect"), ("ReplicationPad1d", "replicate")])
def test_streamed_bf16_start_of_stream_padding(pad, mode, device):
    """Reflect / replicate start-of-stream context against the padded float64 oracle of the rounded operands; the fused
    pre-activation, bias, an addend, out_mul and tanh ride along.  (The bf16 image of a reflect-padded layer is packed
    through a zero-padded descriptor of the same geometry.)"""
    g = torch.Generator().manual_seed(6)
    x = _bf16r(torch.randn(2, 24, 50, generator=g))
    add = torch.randn(2, 40, 50, generator=g)
    w = _bf16r(torch.randn(40, 24, 5, generator=g) / 120 ** 0.5)
    b = torch.randn(40, generator=g)
    xa = _bf16r(F.leaky_relu(x, 0.2))
    xp = F.pad(xa.double(), (12, 0), mode=mode)
    ref = torch.tanh((F.conv1d(xp, w.double(), b.double(), dilation=3) + add.double()) * 0.5)
    conv = layers.CausalConv1d(24, 40, 5, dilation=3, pad=pad, pad_params={})
    _set(conv.conv, w, b)
    conv = conv.to(device)
    for pieces in ((14, 1, 7, 2, 13, 13), (50,), (13,) + (1,) * 37):  # reflect mirrors 12 columns: first piece >= 13
        y = _stream_layer(conv, x.to(device), pieces, add.to(device), pre_act="leaky_relu", pre_slope=0.2, out_mul=0.5,
                          post_act="tanh")
        err = _rel_err(y, ref)
        print(mode, pieces[:4], f"rel-to-max error {err:.3e}")
        assert err <= RTOL
    if mode == "reflect":  # too short a first piece cannot be mirrored: an error, not garbage
        with pytest.raises(RuntimeError, match="reflect"):
            conv.stream_forward(x[..., :12].contiguous().to(device), None, torch.empty(conv.history_shape(2), device=device),
                                precision="bf16")


@pytest.mark.parametrize("pad,params,mode", [("ReplicationPad1d", {}, "replicate"), ("ConstantPad1d", {"value": 0.0}, "constant")])
def test_streamed_bf16_transposed_start_of_stream(pad, params, mode, device):
    g = torch.Generator().manual_seed(7)
    x = _bf16r(torch.randn(2, 24, 30, generator=g))
    w = _bf16r(torch.randn(24, 12, 8, generator=g) / 48 ** 0.5)
    b = torch.randn(12, generator=g)
    ref = _transposed_ref(x, w, b, 4, mode)
    up = layers.CausalConvTranspose1d(24, 12, 8, 4, pad=pad, pad_params=params)
    _set(up.deconv, w, b)
    up = up.to(device)
    for pieces in ((1, 7, 2, 13, 7), (30,), (1,) * 30):
        y = _stream_layer(up, x.to(device), pieces)
        assert y.shape[-1] == 30 * 4
        err = _rel_err(y, ref)
        print("transposed start", mode, pieces[:4], f"rel-to-max error {err:.3e}")
        assert err <= RTOL


def test_bf16_history_buffers_must_be_distinct(device):
    conv = layers.CausalConv1d(8, 8, 3).to(device)
    h = torch.zeros(conv.history_shape(1), device=device)
    with pytest.raises(RuntimeError, match="distinct"):
        conv.stream_forward(torch.zeros(1, 8, 4, device=device), h, h, precision="bf16")
    with pytest.raises(ValueError, match="precision"):
        conv.stream_forward(torch.zeros(1, 8, 4, device=device), None, h, precision="fp16")


# ---- 4. partition invariance, bit for bit -----------------------------------------------------------------------------
def _load(cls, cfg, seed, g_scale, device, pqmf=False):
    m = cls(**cfg)
    sd = synth_for(m, seed, g_scale)
    m.load_state_dict(sd)
    if pqmf:
        m.pqmf = layers.PQMF(subbands=cfg["out_channels"])
    return m.to(device).eval(), sd


def _stream(model, c, pieces, **kw):
    """Push c (B, C, T) in ``pieces`` frames at a time, flush -> (B, T * up)."""
    assert sum(pieces) == c.shape[-1]
    s = kw.pop("stream", None) or CausalStream(model, batch=c.shape[0], **kw)
    feats = c.transpose(1, 2).contiguous()
    outs, t = [], 0
    for n in pieces:
        outs.append(s.push(feats[:, t:t + n]))
        t += n
    outs.append(s.flush())
    s.close()
    out = torch.cat(outs, -1)
    assert s.frames_in == s.frames_out == c.shape[-1] and s.samples_out == out.shape[1] == c.shape[-1] * s.up
    return out


FAMILIES = {
    "hifigan_causal": (models.HiFiGANGenerator, synth.HIFIGAN_CAUSAL, 3, 1.0, False),
    "melgan_causal": (models.MelGANGenerator, synth.MELGAN_CAUSAL, 4, synth.MELGAN_G_SCALE, False),
    "mb_melgan_causal": (models.MelGANGenerator, MB_CAUSAL, 31, synth.MELGAN_G_SCALE, True),
}


def _partitions(frames, warm):
    return [(frames,), (warm,) + (1,) * (frames - warm), (warm, 1, 5, 1, 17, 3, frames - warm - 27),
            (warm + 2, 9, 1, 1, frames - warm - 13)]


def _check_partition_invariance(family, device):
    cls, cfg, seed, scale, pqmf = FAMILIES[family]
    model, _ = _load(cls, cfg, seed, scale, device, pqmf)
    warm, frames = CausalStream.required_warmup_frames(model), 40
    c = torch.randn(3, 80, frames, generator=torch.Generator().manual_seed(9)).to(device)
    parts = _partitions(frames, warm)
    one = _stream(model, c[:2], parts[0], use_graph=False, precision="bf16")
    assert torch.isfinite(one).all() and one.abs().max() > 1e-3
    for p in parts[1:]:
        y = _stream(model, c[:2], p, use_graph=False, precision="bf16")
        assert torch.equal(y, one), (family, p[:4], max_abs(y, one))
    for p in ((warm,) + (3,) * ((frames - warm) // 3), parts[2]):  # graph replay: the same bits as eager
        assert torch.equal(_stream(model, c[:2], p, use_graph=True, precision="bf16"), one), (family, "graph", p[:4])
    # B = 3 lock-step streams equal three single ones
    together = _stream(model, c, parts[2], use_graph=False, precision="bf16")
    assert torch.equal(together[:2], one)
    for i in range(3):
        alone = _stream(model, c[i:i + 1], parts[3], use_graph=False, precision="bf16")
        assert torch.equal(alone[0], together[i]), (family, i)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_bf16_partition_invariance_bit_for_bit(family, device):
    _check_partition_invariance(family, device)


def test_bf16_partition_invariance_with_poisoned_lds(device):
    with poison_lds():
        for family in FAMILIES:
            _check_partition_invariance(family, device)


def test_bf16_v1_geometry_partition_invariance(device):
    """8 .. 6144 columns per push at the V1 widths: every tile of the kernel, chosen by n, on the same frames."""
    model = models.HiFiGANGenerator(**HIFIGAN_V1_CAUSAL)
    model.load_state_dict(synth_for(model, 11, 1.25))
    model.remove_weight_norm()
    model = model.to(device).eval()
    c = torch.randn(1, 80, 24, generator=torch.Generator().manual_seed(10)).to(device)
    ref = _stream(model, c, (24,), use_graph=False, precision="bf16")
    assert torch.isfinite(ref).all() and ref.abs().max() > 1e-3
    for p in ((8,) * 3, (1, 2, 4, 17), (1,) * 24):
        assert torch.equal(_stream(model, c, p, use_graph=False, precision="bf16"), ref), p[:4]
    assert torch.equal(_stream(model, c, (8,) * 3, use_graph=True, precision="bf16"), ref)


def test_bf16_melgan_recipe_width_partition_invariance(device):
    """256 / 128 channels through the 1 x 1 layers, 8 and 16 columns per frame; batched streams equal single ones."""
    model, _ = _load(models.MelGANGenerator, MELGAN_WIDE_CAUSAL, 21, synth.MELGAN_G_SCALE, device)
    frames, warm = 24, CausalStream.required_warmup_frames(model)
    assert warm == 7
    c = torch.randn(3, 80, frames, generator=torch.Generator().manual_seed(22)).to(device)
    whole = [_stream(model, c[i:i + 1], (frames,), use_graph=False, precision="bf16") for i in range(3)]
    assert whole[0].abs().max() > 1e-3
    for p in ((8,) * 3, (warm,) + (1,) * (frames - warm), (warm, 1, 16), (9, 2, 13)):
        y = _stream(model, c[:1], p, use_graph=False, precision="bf16")
        assert torch.equal(y, whole[0]), (p[:4], max_abs(y, whole[0]))
    assert torch.equal(_stream(model, c[:1], (8,) * 3, use_graph=True, precision="bf16"), whole[0])
    together = _stream(model, c, (9, 2, 13), use_graph=False, precision="bf16")
    for i in range(3):
        assert torch.equal(together[i], whole[i][0]), i


# ---- 5. whole generator, statistical ---------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["hifigan_causal", "melgan_causal"])
def test_bf16_stream_error_is_the_emulations_error(family, device):
    """rms(stream_bf16 - oracle_fp32) <= FACTOR * rms(emulation - oracle_fp32); the emulation is the causal CPU oracle
    with every convolution's operands rounded (no predicate), as in the stream.  No sample is left out."""
    cls, cfg, seed, scale, _ = FAMILIES[family]
    model, sd = _load(cls, cfg, seed, scale, device)
    c = synth.synth_input("c", (2, 80, 36), seed=36)
    oracle = torch_cpu.hifigan_generator_causal if family == "hifigan_causal" else torch_cpu.melgan_generator_causal
    kw = dict(cfg, upsample_scales=tuple(cfg["upsample_scales"]))
    with torch.no_grad():
        ref = oracle(sd, c, **kw)
        with bf16_operands() as stats:
            emu = oracle(sd, c, **kw)
    assert stats["untouched"] == 0 and stats["rounded"] == len(list(each_conv(model)))
    y = _stream(model, c.to(device), (9, 8, 8, 1, 10), precision="bf16").cpu()
    assert torch.isfinite(y).all()
    e_gpu, e_emu = rms(y - ref[:, 0]), rms(emu - ref)
    print(f"{family}: rms(stream_bf16 - oracle) {e_gpu:.3e}, rms(emulation - oracle) {e_emu:.3e}, ratio {e_gpu / e_emu:.3f}, "
          f"rms(signal) {rms(ref):.3e}")
    assert e_emu > 0
    assert e_gpu <= FACTOR * e_emu


# ---- 6. the mode is really on, and the default is untouched -------------------------------------------------------------
@pytest.mark.parametrize("family", ["hifigan_causal", "melgan_causal"])
def test_bf16_stream_is_really_on_and_default_is_untouched(family, device):
    cls, cfg, seed, scale, _ = FAMILIES[family]
    model, _ = _load(cls, cfg, seed, scale, device)
    never, _ = _load(cls, cfg, seed, scale, device)
    n_convs = len(list(each_conv(model)))
    c = torch.randn(2, 80, 24, generator=torch.Generator().manual_seed(40)).to(device)
    feats = c.transpose(1, 2).contiguous()
    with torch.no_grad():
        whole_never = never(c)
    y32_never = _stream(never, c, (8, 8, 8))

    s = CausalStream(model, batch=2, use_graph=False, precision="bf16")
    assert s.precision == "bf16"
    first = s.push(feats[:, :8])  # (start of stream; the weight images are built here, outside the profiled pushes)
    with ops.profile() as prof:
        second = s.push(feats[:, 8:16])
    assert prof.results[BF16_STREAM]["launches"] == n_convs, prof.results
    assert not any(k in prof.results for k in OTHER_CONVS), prof.results
    y16 = torch.cat([first, second, s.push(feats[:, 16:])], -1)
    assert torch.isfinite(y16).all() and not torch.equal(y16, y32_never)
    assert torch.equal(_stream(model, c, (8, 8, 8), precision="bf16"), y16)  # deterministic; graph replay = eager

    # the default stream built afterwards on the same model: the fp32 kernel, bit-identical to a model that never saw bf16
    assert all(cv.precision == "fp32" for cv in each_conv(model))
    s32 = CausalStream(model, batch=2, use_graph=False)
    assert s32.precision == "fp32" and CausalStream(model, batch=2, precision="fp32").precision == "fp32"
    s32.push(feats[:, :8])
    with ops.profile() as prof:
        s32.push(feats[:, 8:16])
    assert prof.results[FP32_STREAM]["launches"] == n_convs and BF16_STREAM not in prof.results, prof.results
    assert torch.equal(_stream(model, c, (8, 8, 8)), y32_never)
    assert torch.equal(_stream(model, c, (8, 8, 8), precision="fp32"), y32_never)
    with torch.no_grad():
        assert torch.equal(model(c), whole_never)


def test_bf16_and_fp32_streams_share_their_state(device):
    """History is raw fp32 in both: after the same frames the two streams hold bit-identical state in every layer fed
    by the features alone (the input convolution), and state of the same shapes everywhere."""
    cls, cfg, seed, scale, _ = FAMILIES["hifigan_causal"]
    model, _ = _load(cls, cfg, seed, scale, device)
    c = torch.randn(1, 80, 16, generator=torch.Generator().manual_seed(41)).to(device)
    a, b = CausalStream(model, use_graph=False, precision="bf16"), CausalStream(model, use_graph=False)
    for s in (a, b):
        s.push(c[0].t().contiguous())
    assert a.state_bytes == b.state_bytes and a.latency_samples == b.latency_samples
    assert [t.shape for t in a._halves[0]] == [t.shape for t in b._halves[0]]
    assert torch.equal(a._halves[a._cur][0], b._halves[b._cur][0])


# ---- 7. new weights are never replayed ---------------------------------------------------------------------------------
def test_bf16_new_weights_are_never_replayed_from_an_old_graph(device):
    cls, cfg, seed, scale, _ = FAMILIES["hifigan_causal"]
    model, _ = _load(cls, cfg, seed, scale, device)
    c = torch.randn(1, 80, 40, generator=torch.Generator().manual_seed(15)).to(device)
    s = CausalStream(model, use_graph=True, precision="bf16")
    old = _stream(model, c, (8,) * 5, stream=s)
    other = synth_for(models.HiFiGANGenerator(**cfg), 77, 1.1)
    model.load_state_dict(other)
    s.reset()
    new = _stream(model, c, (8,) * 5, stream=s)
    fresh = models.HiFiGANGenerator(**cfg)
    fresh.load_state_dict(other)
    fresh = fresh.to(device).eval()
    assert torch.equal(new, _stream(fresh, c, (8,) * 5, use_graph=True, precision="bf16"))
    assert max_abs(new, old) > 1e-3
    # between two pushes of one chunk size, mid-utterance: the next push runs on the new weights
    s.reset()
    feats = c.transpose(1, 2).contiguous()
    head = [s.push(feats[:, t:t + 8]) for t in (0, 8, 16)]
    model.load_state_dict(synth_for(models.HiFiGANGenerator(**cfg), seed, scale))
    tail = [s.push(feats[:, t:t + 8]) for t in (24, 32)]
    cut = head[0].shape[1] * 3
    assert torch.equal(torch.cat(head, -1), new[:, :cut])
    assert max_abs(torch.cat(tail, -1), new[:, cut:]) > 1e-3
