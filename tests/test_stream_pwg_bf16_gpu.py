"""GPU: the Parallel WaveGAN streams with bf16 operands -- the gated layer's two streaming forms on the bf16 MFMA
(csrc/wavenet_stream_bf16.hip) and ``PWGStream`` / ``PWGLookaheadStream`` with ``precision="bf16"``.

Layer: every stage against float64 on the kernel's OWN inputs to that stage (the method and the bars of
tests/test_wavenet_bf16_gpu.py); the delayed launch against the whole-utterance bf16 layer bit for bit; the causal launch
against the delayed one; the residual is fp32; the state is the fp32 launch's bit for bit; partitions, batch and repeated
launches change no bit.  Generator: any partition gives the same bits, graph replay equals eager, and the error against
the fp32 CPU oracle is the CPU emulation's error (the bars of tests/test_pwg_bf16_gpu.py)."""
import functools
import math
import random

import pytest
import torch
import torch.nn.functional as F

from oracle import torch_cpu
from parallelwavegan_amd import models, ops
from parallelwavegan_amd.layers.causal_conv import lookahead_window
from parallelwavegan_amd.layers.conv import each_conv
from parallelwavegan_amd.utils import PWGLookaheadStream, PWGStream, set_inference_precision
from tests import test_stream_pwg_gpu as causal_t
from tests import test_stream_pwg_lookahead_gpu as look_t
from tests.bf16_emulation import bf16_operands, rms
from tests.golden import synth
from tests.test_pwg_bf16_gpu import LOWER, UPPER
from tests.test_stream_pwg_lookahead_gpu import B, DEEP, DILATIONS, EXTRA, PARTITIONS, SKIP_SCALE, SMALL, T
from tests.test_wavenet_bf16_gpu import RTOL, _bf16r, _half_ulp_bf16, _rel
from tests.util import load_golden, poison_lds, synth_for

pytestmark = pytest.mark.gpu

assert (B, T, DILATIONS, PARTITIONS) == (causal_t.B, causal_t.T, causal_t.DILATIONS, causal_t.PARTITIONS)
assert (B, T, DILATIONS, RTOL, LOWER, UPPER) == (2, 1200, (1, 4, 512), 3e-5, 0.5, 2.0)

BF16_LAYER, BF16_LAYER_DELAYED = "wavenet_stream_bf16_kernel", "wavenet_stream_bf16_delayed_kernel"
BF16_CONV, BF16_CONV_DELAYED = "conv1d_stream_bf16_kernel", "conv1d_stream_bf16_delayed_kernel"
OTHER_LAUNCHES = ("stretch_conv_stream_kernel", "delay_line_kernel", "normalize_transpose_kernel")


# ---- the layer: one runner for both forms --------------------------------------------------------------------------
def _nan(shape, device):
    return [torch.full(shape, float("nan"), device=device) for _ in range(2)]


def _biases(blk):
    return [cv.bias.detach() for cv in (blk.conv, blk.conv1x1_skip, blk.conv1x1_out)]


def _desc(blk, nb, n, causal, skip_scale=SKIP_SCALE):
    return ops.make_wavenet_desc(nb, n, blk.conv.dilation, causal=causal, out_mul=math.sqrt(0.5), skip_mul=skip_scale)


def _run(blk, x, c, skips, parts, c_delay=None, total=None, check_state=False):
    """Stream (x, c, skips) through the bf16 launch of ``blk``'s weights in pieces, with ``save`` -> dict of x, s, z, g
    over all columns.  ``c_delay`` None: the causal form; else the delayed form with the windows of
    ``lookahead_window(d, 1, n, pos, total)``.  Every state buffer starts as NaN.  ``check_state``: after every piece the
    history (and the skip line) equal those the fp32 launch writes from the same inputs, bit for bit, and the last
    columns of the concatenation."""
    nb, d, dev = x.shape[0], blk.conv.dilation, x.device
    causal = c_delay is None
    img, img32, bias = blk.stream_image_bf16(), blk.stream_image(), _biases(blk)
    hist, sline = _nan((nb, 64, 2 * d), dev), _nan((nb, 64, d), dev)
    cline = _nan((nb, 80, (c_delay or 0) + 5), dev)
    h32, s32 = _nan((nb, 64, 2 * d), dev)[0], _nan((nb, 64, d), dev)[0]
    want_h, want_s = torch.zeros_like(hist[0]), torch.zeros_like(sline[0])
    outs, pos, cur = [], 0, 0
    for i, n in enumerate(parts):
        xp, cp = x[:, :, pos:pos + n].contiguous(), c[:, :, pos:pos + n].contiguous()
        sp = None if skips is None else skips[:, :, pos:pos + n].contiguous()
        first = i == 0
        h_in, l_in, s_in = (None if first else buf[cur] for buf in (hist, cline, sline))
        desc = _desc(blk, nb, n, causal)
        if causal:
            outs.append(ops.wavenet_stream_forward_bf16(desc, xp, cp, sp, h_in, hist[1 - cur], img, *bias, save=True))
            if check_state:
                h32.fill_(float("nan"))
                ops.wavenet_stream_forward(desc, xp, cp, sp, h_in, h32, img32, *bias)
        else:
            valid = lookahead_window(d, 1, n, pos, total)
            outs.append(ops.wavenet_stream_delayed_forward_bf16(desc, xp, cp, l_in, c_delay, sp, (s_in, sline[1 - cur]), h_in,
                                                                hist[1 - cur], img, *bias, valid, save=True))
            assert ops.delay_line_forward(cp, l_in, cline[1 - cur]) is None
            if check_state:
                h32.fill_(float("nan"))
                s32.fill_(float("nan"))
                ops.wavenet_stream_delayed_forward(desc, xp, cp, l_in, c_delay, sp, (s_in, s32), h_in, h32, img32, *bias, valid)
        cur = 1 - cur
        if check_state:
            want_h = torch.cat([want_h, xp], -1)[..., -2 * d:]
            assert torch.equal(hist[cur], h32) and torch.equal(hist[cur], want_h), ("history", i, n)
            if not causal and sp is not None:
                want_s = torch.cat([want_s, sp], -1)[..., -d:]
                assert torch.equal(sline[cur], s32) and torch.equal(sline[cur], want_s), ("skip line", i, n)
        pos += n
    assert pos == x.shape[-1]
    return {k: torch.cat([o[j] for o in outs], -1) for j, k in enumerate(("x", "s", "z", "g"))}


def _case(form, d, device):
    """(block on the device, x, c, skips on the device): the seeded cases of the fp32 stream tests."""
    mod = causal_t if form == "causal" else look_t
    case = mod._layer_case(d)
    return (mod._block(d, device),) + tuple(case[k].to(device) for k in ("x", "c", "skips"))


_STREAMED = {}


def _streamed(form, d, extra, device):
    """Every partition of the layer case through the bf16 launch, once (state checked after every piece)."""
    key = (form, d, extra)
    if key not in _STREAMED:
        blk, x, c, skips = _case(form, d, device)
        c_delay = None if form == "causal" else d + extra
        _STREAMED[key] = [_run(blk, x, c, skips, parts, c_delay, check_state=True) for parts in PARTITIONS]
    return _STREAMED[key]


FORMS = [("causal", 0), ("delayed", 0), ("delayed", EXTRA)]


# ---- 1. stages against float64 on the kernel's own inputs ----------------------------------------------------------
def _effective_bf16(blk):
    """The four effective weights as the packer rounds them: fp32 ``w * scale``, then bf16 -> float64 on the CPU."""
    out = []
    for cv in blk.fused_convs():
        h = cv.prepared()
        w = h.w if h.scale is None else h.w * h.scale.view(-1, 1, 1)
        out.append(_bf16r(w.detach().float().cpu().reshape(cv.out_channels, cv.in_channels, -1)).double())
    return out


def _stage_errors(blk, x, c, skips, out, c_delay, lo=0):
    """(z, g, skips, x) errors of a streamed run, each against float64 on the kernel's own inputs to that stage (the
    method of tests/test_wavenet_bf16_gpu.py::stage_errors).  Causal taps over the zero-padded past; the delayed form
    reads the conditioning ``c_delay`` late and the residual and the skip sum ``d`` late, and stores zeros in front of
    column ``lo``."""
    d = blk.conv.dilation
    x, c, out = x.cpu(), c.cpu(), {k: v.cpu() for k, v in out.items()}
    w_d, w_a, w_s, w_o = _effective_bf16(blk)
    b_d, b_s, b_o = (b.cpu().double() for b in _biases(blk))
    late = lambda t, k: F.pad(t, (k, 0))[..., :t.shape[-1]]  # noqa: E731
    z64 = (F.conv1d(F.pad(_bf16r(x).double(), (2 * d, 0)), w_d, b_d, dilation=d)
           + F.conv1d(late(_bf16r(c).double(), c_delay or 0), w_a))
    zk, gk = out["z"].double(), out["g"].double()
    g64 = torch.tanh(zk[:, :64]) * torch.sigmoid(zk[:, 64:])
    assert torch.equal(_bf16r(out["g"]), out["g"]), "g_out holds values that are not bf16-representable"
    g_excess = ((gk - g64).abs() - _half_ulp_bf16(g64)).max().item() / g64.abs().max().item()
    shift = 0 if c_delay is None else d
    addend = 0.0 if skips is None else late(skips.cpu().double(), shift)
    s64 = (F.conv1d(gk, w_s, b_s) + addend) * SKIP_SCALE
    x64 = (F.conv1d(gk, w_o, b_o) + late(x.double(), shift)) * math.sqrt(0.5)
    for ref in (s64, x64):
        ref[..., :lo] = 0.0
    for name, t in out.items():
        assert torch.isfinite(t).all(), name
        assert name in ("z", "g") or float(t[..., :lo].abs().max() if lo else 0.0) == 0.0, name
    return {"z": _rel(out["z"], z64), "g_excess_over_half_ulp": g_excess, "skips": _rel(out["s"], s64), "x": _rel(out["x"], x64)}


@pytest.mark.parametrize("form,extra", FORMS)
@pytest.mark.parametrize("d", DILATIONS)
def test_stages_match_float64(d, form, extra, device):
    """Figures on an MI355X: DESIGN.md s11.7."""
    blk, x, c, skips = _case(form, d, device)
    c_delay, lo = (None, 0) if form == "causal" else (d + extra, d)
    runs = _streamed(form, d, extra, device)
    cases = [("one launch", skips, runs[1]), ("pieces", skips, runs[0]),
             ("one launch, no skips", None, _run(blk, x, c, None, PARTITIONS[1], c_delay)),
             ("pieces, no skips", None, _run(blk, x, c, None, PARTITIONS[0], c_delay))]
    for what, sk, out in cases:
        e = _stage_errors(blk, x, c, sk, out, c_delay, lo)
        print(f"{form} d={d} c_delay={c_delay} {what}: {e}")
        assert e["z"] <= RTOL, (what, e)
        assert e["g_excess_over_half_ulp"] <= RTOL, (what, e)
        assert e["skips"] <= RTOL, (what, e)
        assert e["x"] <= RTOL, (what, e)


# ---- 2. the delayed launch is the whole-utterance bf16 layer, bit for bit ------------------------------------------
@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("d", DILATIONS)
def test_delayed_launch_is_the_whole_utterance_bf16_layer(d, poison, device):
    blk, x, c, skips = _case("delayed", d, device)
    assert torch.equal(blk.stream_image_bf16(), blk.fused_image_bf16())
    whole = ops.wavenet_bf16_layer_forward(_desc(blk, B, T, False), x, c, skips, blk.fused_image_bf16(), *_biases(blk),
                                           save=True)
    tail = lambda t: torch.cat([t, torch.zeros(*t.shape[:2], d, device=device)], -1)  # noqa: E731
    for parts in PARTITIONS:
        parts = parts + (d,)  # the flush: d more columns, of which none is valid input
        if poison:
            with poison_lds():
                out = _run(blk, tail(x), tail(c), tail(skips), parts, d, total=T)
        else:
            out = _run(blk, tail(x), tail(c), tail(skips), parts, d, total=T)
        for name, want in (("z", whole[2]), ("g", whole[3]), ("x", whole[0]), ("s", whole[1])):
            assert torch.equal(out[name][..., d:], want), (name, len(parts), _rel(out[name][..., d:], want))
        for name in ("x", "s"):
            assert float(out[name][..., :d].abs().max()) == 0.0, name


# ---- 3. causal against delayed -------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DILATIONS)
def test_causal_launch_equals_the_delayed_one_without_delays(d, device):
    """c_delay = 0, no skip input, full window: the same z, the same g, the same skip epilogue."""
    blk, x, c, _ = _case("delayed", d, device)
    img, bias = blk.stream_image_bf16(), _biases(blk)
    hist = [_nan((B, 64, 2 * d), device) for _ in range(2)]  # [form][ping-pong]
    pos, cur = 0, None
    for n in PARTITIONS[0]:
        nxt = 0 if cur is None else 1 - cur
        xp, cp = x[:, :, pos:pos + n].contiguous(), c[:, :, pos:pos + n].contiguous()
        h_in = [None if cur is None else h[cur] for h in hist]
        xc, sc, zc, gc = ops.wavenet_stream_forward_bf16(_desc(blk, B, n, True), xp, cp, None, h_in[0], hist[0][nxt], img,
                                                         *bias, save=True)
        xd, sd, zd, gd = ops.wavenet_stream_delayed_forward_bf16(_desc(blk, B, n, False), xp, cp, None, 0, None, (None, None),
                                                                 h_in[1], hist[1][nxt], img, *bias, (0, n), save=True)
        assert torch.isfinite(sc).all()
        assert torch.equal(zc, zd) and torch.equal(gc, gd) and torch.equal(sc, sd), (pos, n)
        assert torch.equal(hist[0][nxt], hist[1][nxt])
        assert not torch.equal(xc, xd)  # (the residual differs: x[n] against the middle tap)
        cur, pos = nxt, pos + n


# ---- 4. the residual is fp32 ---------------------------------------------------------------------------------------
def test_residual_is_the_fp32_input_not_its_rounded_copy(device):
    """As tests/test_wavenet_bf16_gpu.py: rebuilding x_out with bf16(residual) must miss the bar.  Causal: x[n].  Delayed
    (d = 512, pieces of 600): the middle tap, columns [0, 512) of the second piece from the history, the rest from the
    chunk."""
    for form, d, parts in (("causal", 4, (600, 600)), ("delayed", 512, (600, 600))):
        blk, x, c, skips = _case(form, d, device)
        out = _run(blk, x, c, skips, parts, None if form == "causal" else d)
        w_o = _effective_bf16(blk)[3]
        conv = F.conv1d(out["g"].cpu().double(), w_o, blk.conv1x1_out.bias.detach().cpu().double())
        res = x.cpu() if form == "causal" else F.pad(x.cpu(), (d, 0))[..., :T]
        right, wrong = (conv + res.double()) * math.sqrt(0.5), (conv + _bf16r(res).double()) * math.sqrt(0.5)
        got = out["x"].cpu()
        spans = ((0, T),) if form == "causal" else ((600, 600 + d), (600 + d, T))
        for lo, hi in spans:
            r, w = _rel(got[..., lo:hi], right[..., lo:hi]), _rel(got[..., lo:hi], wrong[..., lo:hi])
            print(f"{form} columns [{lo}, {hi}): fp32 residual {r:.3e}, rounded residual {w:.3e}")
            assert r <= RTOL < w, (form, lo, hi, r, w)


# ---- 5. state, 6. invariance ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,extra", FORMS)
@pytest.mark.parametrize("d", DILATIONS)
def test_state_partitions_and_batch(d, form, extra, device):
    """After every piece of every partition the bf16 launch's history and skip line are the fp32 launch's, bit for bit,
    and the last columns of the concatenation (checked inside ``_run``); all partitions give identical bits; lock-step
    items give the bits of single ones; a second run gives the same bits."""
    runs = _streamed(form, d, extra, device)
    for out in runs[1:]:
        for k in ("x", "s", "z", "g"):
            assert torch.equal(out[k], runs[0][k]), (k, form, d)
    blk, x, c, skips = _case(form, d, device)
    c_delay = None if form == "causal" else d + extra
    again = _run(blk, x, c, skips, PARTITIONS[0], c_delay)
    for k in ("x", "s", "z", "g"):
        assert torch.equal(again[k], runs[0][k]), k
    for b in range(B):
        single = _run(blk, x[b:b + 1], c[b:b + 1], skips[b:b + 1], PARTITIONS[0], c_delay)
        for k in ("x", "s", "z", "g"):
            assert torch.equal(single[k], runs[0][k][b:b + 1]), (k, b)


def test_skips_may_alias_in_the_causal_form_only(device):
    d, n = 4, 70
    blk, x, c, skips = _case("causal", d, device)
    x, c, skips = (t[:, :, :n].contiguous() for t in (x, c, skips))
    h = _nan((B, 64, 2 * d), device)
    sep = blk.stream_forward(x, c, None, h[0], skips=skips, skip_scale=SKIP_SCALE, precision="bf16")
    own = skips.clone()
    xo, so = blk.stream_forward(x, c, None, h[1], skips=own, skip_scale=SKIP_SCALE, inplace_skips=True, precision="bf16")
    assert so.data_ptr() == own.data_ptr() and torch.equal(so, sep[1]) and torch.equal(xo, sep[0])
    with pytest.raises(RuntimeError, match="distinct"):
        blk.stream_forward(x, c, h[0], h[0], precision="bf16")
    nc, xd, cd, sd = _case("delayed", d, device)
    xd, cd, sd = (t[:, :, :n].contiguous() for t in (xd, cd, sd))
    line = _nan((B, 64, d), device)
    with pytest.raises(RuntimeError, match="skip_line_in and skip_line_out must be distinct"):
        nc.lookahead_forward(xd, cd, None, d, (None, h[0]), sd, (line[0], line[0]), precision="bf16")
    with pytest.raises(RuntimeError, match="conditioning line"):
        nc.lookahead_forward(xd, cd, torch.zeros(B, 80, d - 1, device=device), d, (None, h[0]), sd, (None, line[0]),
                             precision="bf16")


@pytest.mark.parametrize("form", ["causal", "delayed"])
def test_nan_input_reaches_exactly_its_three_taps(form, device):
    """Round-to-nearest-even keeps NaN a NaN: x[0, 5, 100] is read by the taps of columns 100, 100 + d and 100 + 2 d."""
    d, n = 2, 200
    blk, x, c, _ = _case(form, 4, device)
    x, c = x[:1, :, :n].clone(), c[:1, :, :n].contiguous()
    x[0, 5, 100] = float("nan")
    img, bias, h = blk.stream_image_bf16(), _biases(blk), _nan((1, 64, 2 * d), device)[0]
    desc = ops.make_wavenet_desc(1, n, d, causal=form == "causal", out_mul=math.sqrt(0.5))
    if form == "causal":
        z = ops.wavenet_stream_forward_bf16(desc, x, c, None, None, h, img, *bias, save=True)[2]
    else:
        z = ops.wavenet_stream_delayed_forward_bf16(desc, x, c, None, d, None, (None, None), None, h, img, *bias, save=True)[2]
    assert torch.isnan(z[0]).any(0).nonzero().flatten().tolist() == [100, 100 + d, 100 + 2 * d]


# ---- 7. the generators ---------------------------------------------------------------------------------------------
def _pieces(frames, seed):
    """A partition of ``frames`` into pieces of 1 - 5 frames from a seeded generator."""
    rnd, parts = random.Random(seed), []
    while sum(parts) < frames:
        parts.append(rnd.randint(1, min(5, frames - sum(parts))))
    return tuple(parts)


@functools.lru_cache(maxsize=None)
def _generator_case(name):
    """(cfg, state dict, mel frames (B, 80, n), noise, fp32 CPU oracle (B, n * up), rms of the bf16 emulation's error): on
    the CPU, once, never modified.  The oracle is ``torch_cpu.pwg_generator`` on the replicate-padded mel, or
    ``pwg_generator_causal``; the emulation is the same oracle under ``bf16_operands()``: conv_in, first_conv, four
    convolutions per layer and the two last ones are rounded (the stretch stages are 2-D convolutions and stay fp32, as
    in the stream)."""
    if name == "causal":
        cfg, seed, n, nb, g_scale = synth.PWG_CAUSAL, 43, 18, 2, 1.0
    elif name == "small":
        cfg, seed, n, nb, g_scale = SMALL, 41, 18, 2, 1.0
    elif name == "deep":
        cfg, seed, n, nb, g_scale = DEEP, 77, 80, 2, 1.0
    else:
        gold = load_golden("pwg_v1")
        n, seed = (int(v) for v in gold["meta"])
        cfg, nb, g_scale = {}, 1, synth.PWG_G_SCALE
    m = models.ParallelWaveGANGenerator(**cfg)
    if name == "v1":  # the golden's own inputs
        sd = synth.synth_state_dict(m.state_dict(), seed=seed, g_scale=g_scale)
        frames = synth.synth_input("c", (1, 80, n + 4), seed=seed)[:, :, 2:-2].contiguous()
        z = synth.synth_input("z", (1, 1, n * 256), seed=seed)
    else:
        sd = synth_for(m, seed, g_scale)
        frames = synth.synth_input("c", (nb, 80, n), seed=seed)
        z = synth.synth_input("z", (nb, 1, n * 16), seed=seed)
    oracle = torch_cpu.pwg_generator_causal if name == "causal" else torch_cpu.pwg_generator
    padded = F.pad(frames, (2, 2), mode="replicate")
    with torch.no_grad():
        ref = oracle(sd, z, padded, **cfg)
        with bf16_operands() as stats:
            emu = oracle(sd, z, padded, **cfg)
    layers = cfg.get("layers", 30)
    assert stats == {"rounded": 1 + 1 + 4 * layers + 2, "untouched": 0}, stats
    e_emu = rms(emu - ref)
    assert e_emu > 0
    return cfg, sd, frames, z, ref[:, 0], e_emu


def _model(name, device):
    cfg, sd = _generator_case(name)[:2]
    m = models.ParallelWaveGANGenerator(**cfg)
    m.load_state_dict(sd)
    return m.to(device).eval()


def _stream(name, m, batch, use_graph=False, precision="bf16"):
    cls = PWGStream if name == "causal" else PWGLookaheadStream
    return cls(m, batch=batch, use_graph=use_graph, precision=precision)


def _stream_all(name, s, frames, z, parts):
    s.reset()
    if name == "causal":
        return causal_t._push_all(s, frames, z, parts)
    return look_t._stream_all(s, frames, z, parts)


GENERATORS = ["causal", "small", "deep", "v1"]


@pytest.mark.parametrize("name", GENERATORS)
def test_generator_partitions_and_error(name, device):
    """Pieces of 1 - 5 frames give the bits of one push plus flush, and rms(stream_bf16 - oracle_fp32) is LOWER ... UPPER
    times rms(emulation - oracle_fp32).  No sample is left out.  Figures on an MI355X: DESIGN.md s11.7."""
    cfg, sd, frames, z, ref, e_emu = _generator_case(name)
    m = _model(name, device)
    frames, z, n = frames.to(device), z.to(device), frames.shape[-1]
    s = _stream(name, m, frames.shape[0])
    assert s.precision == "bf16" and s.state_bytes == _stream(name, m, frames.shape[0], precision=None).state_bytes
    whole = _stream_all(name, s, frames, z, (n,))
    assert whole.shape == ref.shape and torch.isfinite(whole).all()
    for seed in (1, 2):
        y = _stream_all(name, s, frames, z, _pieces(n, seed))
        assert torch.equal(y, whole), (name, seed)
    e_gpu = rms(whole.cpu() - ref)
    print(f"{name}: rms(stream_bf16 - oracle) {e_gpu:.3e}, rms(emulation - oracle) {e_emu:.3e}, ratio {e_gpu / e_emu:.3f}, "
          f"rms(signal) {rms(ref):.3e}")
    assert LOWER <= e_gpu / e_emu <= UPPER, (name, e_gpu, e_emu)
    assert all(cv.precision == "fp32" for cv in each_conv(m))


@pytest.mark.parametrize("name", ["causal", "small"])
def test_generator_graph_replay_equals_eager(name, device):
    _, _, frames, z, _, _ = _generator_case(name)
    m = _model(name, device)
    frames, z = frames.to(device), z.to(device)
    parts = (2,) * 9  # small: 3 eager start-up pushes (6 >= latency_frames 5), then replays; causal: 1 eager push
    eager = _stream_all(name, _stream(name, m, 2), frames, z, parts)
    sg = _stream(name, m, 2, use_graph=True)
    assert torch.equal(_stream_all(name, sg, frames, z, parts), eager)
    assert set(sg._graphs) == {(2, 80)}
    assert torch.equal(_stream_all(name, sg, frames, z, parts), eager)  # reset() and a second utterance on the same graphs


@pytest.mark.parametrize("name", ["causal", "small"])
def test_generator_bf16_is_really_on_and_the_default_is_untouched(name, device):
    _, _, frames, z, _, _ = _generator_case(name)
    m, never = _model(name, device), _model(name, device)
    frames, z = frames.to(device), z.to(device)
    parts, layers = (6, 6, 6), len(m.conv_layers)
    y32_never = _stream_all(name, _stream(name, never, 2, precision=None), frames, z, parts)
    feats = frames.transpose(1, 2).contiguous()

    def second_push(s):
        s.reset()
        s.push(feats[:, :6], z[:, 0, :96])  # (start of stream; the weight images are built here)
        with ops.profile() as prof:
            s.push(feats[:, 6:12], z[:, 0, 96:192])
        return prof.results

    layer, conv = (BF16_LAYER, BF16_CONV) if name == "causal" else (BF16_LAYER_DELAYED, BF16_CONV_DELAYED)
    s16 = _stream(name, m, 2)
    res = second_push(s16)
    assert res[layer]["launches"] == layers and res[conv]["launches"] == 4, res  # conv_in, first_conv, the two last
    assert set(res) <= {layer, conv} | set(OTHER_LAUNCHES), res
    y16 = _stream_all(name, s16, frames, z, parts)
    assert torch.isfinite(y16).all() and y16.shape == y32_never.shape and not torch.equal(y16, y32_never)
    # the default stream on the same model afterwards: the fp32 kernels, the bits of a model that never saw bf16
    assert all(cv.precision == "fp32" for cv in each_conv(m))
    s32 = _stream(name, m, 2, precision=None)
    assert s32.precision == "fp32" and _stream(name, m, 2, precision="fp32").precision == "fp32"
    res = second_push(s32)
    assert not [k for k in res if "bf16" in k], res
    assert res["wavenet_stream_kernel" if name == "causal" else "wavenet_stream_delayed_kernel"]["launches"] == layers
    assert torch.equal(_stream_all(name, s32, frames, z, parts), y32_never)
    # a model in bf16 mode: the bf16 stream takes it, gives the same bits and leaves the mode alone
    assert set_inference_precision(m, "bf16") > 0
    mode = [cv.precision for cv in each_conv(m)]
    assert "bf16" in mode
    assert torch.equal(_stream_all(name, _stream(name, m, 2), frames, z, parts), y16)
    assert [cv.precision for cv in each_conv(m)] == mode
    with pytest.raises(ValueError, match="bf16"):
        _stream(name, m, 2, precision=None)
