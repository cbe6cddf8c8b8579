"""GPU: stateful PQMF synthesis (csrc/pqmf.hip pwg_pqmf_up_stream, PQMF.stream_synthesis) and the causal multi-band
MelGAN stream on top of it (utils.CausalStream) -- the kernel against the float64 reference form and bit for bit against
the whole-utterance PQMF.synthesis for every partition, the streamed model against the oracle and against the package's
own forward, and the state handling (delay, flush, reset, graphs); plus ChunkedSynthesizer / receptive_field_frames on a
multi-band model."""
import pytest
import torch
import torch.nn.functional as F

from oracle import torch_cpu
from parallelwavegan_amd import layers, models
from parallelwavegan_amd.utils import CausalStream, streaming
from tests.golden import synth
from tests.test_stream_mb_host import MB_CAUSAL, PARTITIONS
from tests.util import WAVE_TOL, max_abs, poison_lds, synth_for

pytestmark = pytest.mark.gpu

FILTERS = [(4, 62, 0.142, 9.0), (3, 62, 0.15, 9.0), (2, 62, 0.267, 9.0), (8, 62, 0.07, 9.0), (4, 30, 0.142, 9.0),
           (5, 14, 0.12, 7.0), (8, 126, 0.07, 9.0), (4, 8, 0.142, 9.0)]


def _ref_synthesis(pq, y):
    """The reference's two-convolution form in float64 from the layer's own buffers (layers/pqmf.py:133-149)."""
    hs, ud = pq.synthesis_filter.double().cpu(), pq.updown_filter.double().cpu()
    pad, k = pq.taps // 2, pq.subbands
    return F.conv1d(F.pad(F.conv_transpose1d(y.double().cpu(), ud * k, stride=k), (pad, pad)), hs)[:, 0]


def _stream_pqmf(pq, y, pieces):
    """y (B, K, N) through ``pq.stream_synthesis`` in ``pieces`` with ping-pong history (NaN until written), then the
    flush: D zero columns -> (B, K * N)."""
    assert sum(pieces) == y.shape[-1]
    delay = pq.stream_delay_columns
    hist = [torch.full(pq.history_shape(y.shape[0]), float("nan"), device=y.device) for _ in range(2)]
    outs, t, cur = [], 0, None
    for n in tuple(pieces) + (delay,):
        chunk = y[..., t:t + n].contiguous() if t < y.shape[-1] else y.new_zeros(y.shape[0], pq.subbands, delay)
        n_emit = max(0, t + n - delay) - max(0, t - delay)
        if t + n <= delay:
            assert n_emit == 0  # nothing is complete yet: the launch only moves history
        nxt = 0 if cur is None else 1 - cur
        outs.append(pq.stream_synthesis(chunk, None if cur is None else hist[cur], hist[nxt], n_emit))
        assert outs[-1].shape == (y.shape[0], pq.subbands * n_emit)
        cur, t = nxt, t + n
    return torch.cat(outs, -1)


# ---- 1. the kernel ------------------------------------------------------------------------------------------------
def _check_kernel(pq, pieces, device):
    k, total = pq.subbands, sum(pieces)
    y = torch.randn(2, k, total, generator=torch.Generator().manual_seed(1000 * k + total))
    ref = _ref_synthesis(pq, y)
    whole = pq.synthesis(y.to(device))[:, 0]
    out = _stream_pqmf(pq, y.to(device), pieces)
    assert out.shape == (2, k * total)
    err = max_abs(out, ref)
    print("pqmf stream", k, pq.taps, pieces[:4], err)
    assert err <= 2e-6 * max(1.0, ref.abs().max().item())
    assert torch.equal(out, whole), (pieces[:4], max_abs(out, whole))


@pytest.mark.parametrize("subbands, taps, cutoff, beta", FILTERS)
def test_stream_kernel_matches_reference_and_whole_utterance_bits(subbands, taps, cutoff, beta, device):
    pq = layers.PQMF(subbands, taps, cutoff, beta).to(device)
    for pieces in PARTITIONS:
        _check_kernel(pq, pieces, device)


def test_stream_kernel_with_poisoned_lds(device):
    pq = layers.PQMF(4).to(device)
    with poison_lds():
        _check_kernel(pq, (1, 7, 2, 13, 5, 1, 21), device)
        _check_kernel(pq, (3, 1321), device)


# ---- 2. errors ----------------------------------------------------------------------------------------------------
def test_stream_kernel_error_cases(device):
    pq = layers.PQMF(4).to(device)
    y = torch.zeros(1, 4, 20, device=device)
    h = torch.zeros(pq.history_shape(1), device=device)
    with pytest.raises(RuntimeError, match="distinct"):
        pq.stream_synthesis(y, h, h, 20)
    with pytest.raises(RuntimeError, match="n_emit"):
        pq.stream_synthesis(y, None, h, 21)
    with pytest.raises(RuntimeError, match="n_emit"):
        pq.stream_synthesis(y, None, h, -1)


# ---- 3. model level -----------------------------------------------------------------------------------------------
def _mb_model(device, seed=31, **over):
    m = models.MelGANGenerator(**dict(MB_CAUSAL, **over))
    sd = synth_for(m, seed, synth.MELGAN_G_SCALE)
    m.load_state_dict(sd)
    m.pqmf = layers.PQMF(subbands=4)
    return m.to(device).eval(), sd


def _gain(pq):
    """G = max_r sum_k sum_d |g[k][r + pad - dK]| from the layer's own filter: the most one unit of error in the
    sub-bands can add to a sample."""
    g, pad, k = pq._synthesis_weight[:, 0].double().cpu(), pq.taps // 2, pq.subbands
    return max(sum(g[:, m].abs().sum().item() for m in range(pq.taps + 1) if (m - r - pad) % k == 0) for r in range(k))


def _stream(model, c, pieces, sizes=None, **kw):
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
    if sizes is not None:
        sizes.extend(o.shape[1] for o in outs)
    out = torch.cat(outs, -1)
    assert s.frames_in == s.frames_out == c.shape[-1] and s.samples_out == out.shape[1] == c.shape[-1] * s.up
    return out


@pytest.fixture(scope="module")
def mb(device):
    model, sd = _mb_model(device)
    c = torch.randn(2, 80, 40, generator=torch.Generator().manual_seed(32))
    one = _stream(model, c.to(device), (40,), use_graph=False)
    return model, sd, c, one


def test_multiband_stream_geometry(mb):
    model, _, _, one = mb
    s = CausalStream(model, batch=2)
    assert s.up == model.upsample_factor * 4 == 64 and s.latency_samples == 32 and s.warmup_frames == 7
    assert one.shape == (2, 40 * 64) and torch.isfinite(one).all() and one.abs().max() > 1e-3
    full_band = models.MelGANGenerator(**synth.MELGAN_CAUSAL).to(one.device)
    s1 = CausalStream(full_band, use_graph=False)
    assert s1.latency_samples == 0 and s1.up == full_band.upsample_factor
    assert s1.push(torch.zeros(8, 80)).shape == (1, 8 * s1.up) and s1.flush().shape == (1, 0)


def test_multiband_partition_invariance_bit_for_bit(mb, device):
    model, _, c, one = mb
    c = c.to(device)
    sizes = []
    by_frame = _stream(model, c, (7,) + (1,) * 33, sizes=sizes, use_graph=False)
    # 7 frames = 112 columns: the first emission is short by the delay; then n * up per push; the flush returns the tail
    assert sizes == [7 * 64 - 32] + [64] * 33 + [32]
    assert torch.equal(by_frame, one)
    for p in ((7, 1, 5, 1, 17, 3, 6), (9, 9, 1, 1, 20)):
        assert torch.equal(_stream(model, c, p, use_graph=False), one), p
    for p in ((7,) + (1,) * 33, (7, 1, 5, 1, 17, 3, 6), (10,) * 4):
        assert torch.equal(_stream(model, c, p, use_graph=True), one), ("graph", p[:4])


def test_multiband_stream_matches_oracle_and_whole_utterance_forward(mb, device):
    model, sd, c, one = mb
    gain = _gain(model.pqmf)
    assert abs(gain - 7.83) < 0.01
    ref = torch_cpu.pqmf_synthesis(torch_cpu.melgan_generator_causal(sd, c, upsample_scales=(4, 2, 2), stacks=2))[:, 0]
    err = max_abs(one, ref)
    print("multi-band stream vs oracle", err, "bound", WAVE_TOL * gain)
    assert err <= WAVE_TOL * gain
    with torch.no_grad():
        full = model.pqmf.synthesis(model(c.to(device)))[:, 0]
    err = max_abs(one, full)
    print("multi-band stream vs forward + synthesis", err, "bound", 2e-5 * gain)
    assert err <= 2e-5 * gain


# ---- 4. frames shorter than the PQMF delay ------------------------------------------------------------------------
def test_frames_shorter_than_the_delay(device):
    model, _ = _mb_model(device, seed=33, upsample_scales=[2, 2], pad="ConstantPad1d", pad_params={"value": 0.0})
    frames = 12
    c = torch.randn(1, 80, frames, generator=torch.Generator().manual_seed(34)).to(device)
    assert CausalStream.required_warmup_frames(model) == 1 and model.upsample_factor == 4 < model.pqmf.stream_delay_columns
    one = _stream(model, c, (frames,), use_graph=False)
    for graph in (False, True):
        sizes = []
        y = _stream(model, c, (1,) * frames, sizes=sizes, use_graph=graph)
        assert sizes == [0, 0] + [16] * (frames - 2) + [32] and sum(sizes) == frames * 16
        assert torch.equal(y, one), graph
    s = CausalStream(model, use_graph=False)  # a push that emits nothing yet converts to an empty PCM16 tensor
    pcm = s.push_pcm16(c[0, :, :1].t().contiguous())
    assert pcm.shape == (1, 0) and pcm.dtype == torch.int16


# ---- 5. state -----------------------------------------------------------------------------------------------------
def test_batched_multiband_streams_equal_single_streams(device):
    model, _ = _mb_model(device)
    c = torch.randn(3, 80, 24, generator=torch.Generator().manual_seed(35)).to(device)
    together = _stream(model, c, (8, 1, 7, 8))
    for i in range(3):
        assert torch.equal(_stream(model, c[i:i + 1], (8, 1, 7, 8))[0], together[i]), i


def test_reset_flush_and_pcm16(mb, device):
    model, _, c, _ = mb
    c1, c2 = c[:1].to(device), c[1:].to(device)
    s = CausalStream(model, use_graph=False)
    first = _stream(model, c1, (8,) * 5, stream=s)
    assert s.flush().shape == (1, 0)  # a second flush has nothing left
    with pytest.raises(RuntimeError, match="reset"):
        s.push(c1[0, :, :8].t().contiguous())
    s.reset()
    assert s.frames_in == s.frames_out == s.samples_out == 0
    assert torch.equal(_stream(model, c1, (8,) * 5, stream=s), first)
    # without reset() (and without a flush, after which push raises) the state of another utterance is carried into
    # this one: the first utterance is not reproduced, so the comparison above can fail
    s.reset()
    for t in range(0, 40, 8):
        s.push(c2[0, :, t:t + 8].t().contiguous())
    s.close()
    carried = torch.cat([s.push(c1[0, :, t:t + 8].t().contiguous()) for t in range(0, 40, 8)], -1)
    assert carried.shape[1] == 40 * 64 and max_abs(carried[:, :4 * 64], first[:, :4 * 64]) > 1e-3
    # PCM16
    s.reset()
    feats = c1[0].t().contiguous()
    pcm = torch.cat([s.push_pcm16(feats[t:t + 8]) for t in range(0, 40, 8)] + [streaming.to_pcm16(s.flush())], -1)
    assert pcm.dtype == torch.int16 and torch.equal(pcm, streaming.to_pcm16(first))


def test_new_weights_are_never_replayed_from_an_old_multiband_graph(device):
    model, _ = _mb_model(device)
    gain = _gain(model.pqmf)
    c = torch.randn(1, 80, 32, generator=torch.Generator().manual_seed(36)).to(device)
    s = CausalStream(model, use_graph=True)
    old = _stream(model, c, (8,) * 4, stream=s)
    other = models.MelGANGenerator(**MB_CAUSAL)
    model.load_state_dict(synth_for(other, 77, synth.MELGAN_G_SCALE), strict=False)  # (the PQMF's buffers stay)
    s.reset()
    new = _stream(model, c, (8,) * 4, stream=s)  # the same chunk size: its graphs hold the old weights
    with torch.no_grad():
        full = model.pqmf.synthesis(model(c))[:, 0]
    assert max_abs(new, full) <= 2e-5 * gain
    assert max_abs(new, old) > 1e-3


# ---- 6. ChunkedSynthesizer / receptive field ------------------------------------------------------------------------
class _BandZero(torch.nn.Module):
    def __init__(self, model):
        super().__init__()
        self.model, self.upsample_factor, self.in_channels = model, model.upsample_factor, 80

    def forward(self, c):
        return self.model(c)[:, :1].contiguous()


def test_chunked_synthesizer_and_receptive_field_on_a_multiband_model(mb, device):
    model, _, _, _ = mb
    gain = _gain(model.pqmf)
    left, right = streaming.receptive_field_frames(model)
    assert right == 0 and left > 0
    assert streaming.receptive_field_frames(_BandZero(model)) == (left, 0)
    feat = torch.randn(300, 80, generator=torch.Generator().manual_seed(37)).to(device)
    with torch.no_grad():
        full = model.pqmf.synthesis(model(feat.t().unsqueeze(0).contiguous()))[0, 0]
    for graph in (False, True):
        y = streaming.ChunkedSynthesizer(model, chunk_frames=64, use_graph=graph).synthesize(feat)
        assert y.shape == full.shape == (300 * model.upsample_factor * 4,)
        assert max_abs(y, full) <= 2e-5 * gain
    bare = models.MelGANGenerator(**MB_CAUSAL).to(device).eval()  # sub-bands out, nothing to synthesise them with
    with pytest.raises(ValueError, match="PQMF"):
        streaming.ChunkedSynthesizer(bare, chunk_frames=64, halo=(left, 0), use_graph=False).synthesize(feat)
