"""GPU: utterances of different lengths in one exact Parallel WaveGAN forward: the ragged forms of the
one-launch layer kernels (csrc/wavenet.hip, csrc/wavenet_bf16.hip), ``ParallelWaveGANGenerator.forward_ragged`` and
``utils.PWGRaggedSynthesizer``.

The kernels are compared bit for bit: every item of a ragged launch against the plain op on the item alone (contiguous
crops, ``t = e``), at the same MFMA shape for bf16; nothing at or past an item's end is written (sentinels) and nothing
there is read (NaN).  The generator is compared per item against ``forward`` on the item alone (2e-5: one generator
under two tile configurations, ``ALONE_TOL`` of tests/test_ragged_gpu.py) and against the CPU oracle (``WAVE_TOL``)."""
import functools
import math

import pytest
import torch

from oracle import torch_cpu
from parallelwavegan_amd import ops
from parallelwavegan_amd.models import ParallelWaveGANGenerator
from parallelwavegan_amd.utils import PWGRaggedSynthesizer, set_inference_precision
from parallelwavegan_amd.utils.streaming import RaggedGroup, to_pcm16
from tests.bf16_emulation import bf16_operands, rms
from tests.golden import synth
from tests.test_pwg_melgan_gpu import PWG_G
from tests.util import WAVE_TOL, max_abs, synth_for

pytestmark = pytest.mark.gpu

ALONE_TOL = 2e-5  # one generator under two tile configurations (tests/test_ragged_gpu.py, tests/test_stream_gpu.py)
GUARD, SENTINEL = 64, 12345.0
B = 5


def _bits(t):
    return t.contiguous().view(torch.int32)


class Sentinels:
    """An output view in the middle of a sentinel-filled buffer; unlike ``Guarded`` of tests/test_conv_split_gpu.py it
    expects sentinels to survive INSIDE the view: the ragged layer writes nothing at or past an item's end."""

    def __init__(self, shape, device):
        n = math.prod(shape)
        self.buf = torch.full((GUARD + n + GUARD,), SENTINEL, device=device)
        self.out = self.buf[GUARD:GUARD + n].view(shape)

    def guards_hold(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[-GUARD:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------ layer kernels
PRECISIONS = {"fp32": (False, None), "bf16_32": (True, 32), "bf16_16": (True, 16)}
# (T, rate, frames per item, skips): the ends e = min(frames * rate, T) cover {0, 4, 64, 68, 700, T}: an empty item, one
# inside the first tile, one ending on / 4 past a tile boundary, one in the middle and the clamp (frames * rate > T);
# against the dilations 1, 4, 512 an item shorter than d (both outer taps read only zeros) and one straddling d (700).
# T = 1340 and 1342 are no multiples of the 64-column tile: a partial last tile.  skips: separate buffers, none, or
# updated in place
LAUNCHES = [(1344, 4, (0, 1, 16, 17, 175), "separate"),
            (1344, 4, (400, 175, 0, 17, 16), "none"),
            (1344, 256, (0, 1, 2, 3, 6), "aliased"),
            (1340, 4, (400, 1, 16, 17, 175), "separate"),
            (1342, 4, (400, 1, 16, 17, 175), "separate")]  # (T % 4 != 0: the fp32 kernel's scalar stores)
assert {min(f * r, t) for t, r, fr, _ in LAUNCHES if t == 1344 and r == 4 for f in fr} == {0, 4, 64, 68, 700, 1344}


@functools.lru_cache(maxsize=None)
def _layer_inputs(t):
    g = torch.Generator().manual_seed(t)
    return dict(x=torch.randn(B, 64, t, generator=g), c=torch.randn(B, 80, t, generator=g),
                skips=torch.randn(B, 64, t, generator=g),
                w_dil=torch.randn(128, 64, 3, generator=g) / 192 ** 0.5, w_aux=torch.randn(128, 80, 1, generator=g) / 80 ** 0.5,
                w_skip=torch.randn(64, 64, 1, generator=g) / 8, w_out=torch.randn(64, 64, 1, generator=g) / 8,
                b_dil=torch.randn(128, generator=g), b_skip=torch.randn(64, generator=g), b_out=torch.randn(64, generator=g))


class Layer:
    """One layer's weights on the device and its plain / ragged launches in one precision."""

    def __init__(self, precision, dilation, t, device):
        self.bf16, self.shape = PRECISIONS[precision]
        self.d, self.t, self.device = dilation, t, device
        i = {k: v.to(device) for k, v in _layer_inputs(t).items()}
        self.i = i
        pack = ops.wavenet_bf16_pack_weights if self.bf16 else ops.wavenet_pack_weights
        self.image = pack(self.desc(1, 64), i["w_dil"], None, i["w_aux"], None, i["w_skip"], None, i["w_out"], None)
        self.biases = (i["b_dil"], i["b_skip"], i["b_out"])

    def desc(self, batch, t):
        return ops.make_wavenet_desc(batch, t, self.d, out_mul=math.sqrt(0.5), skip_mul=0.75)

    def plain(self, x, c, skips):
        d = self.desc(x.shape[0], x.shape[2])
        if self.bf16:
            return ops.wavenet_bf16_layer_forward(d, x, c, skips, self.image, *self.biases, mfma_shape=self.shape)[:2]
        return ops.wavenet_layer_forward(d, x, c, skips, self.image, *self.biases)[:2]

    def ragged(self, x, c, skips, table, rate, skips_out=None, x_out=None):
        return ops.wavenet_layer_forward_ragged(self.desc(x.shape[0], x.shape[2]), x, c, skips, table, rate, self.image,
                                                *self.biases, skips_out=skips_out, x_out=x_out, bf16=self.bf16,
                                                mfma_shape=self.shape)

    def inputs_with_nan_tails(self, ends):
        x, c, skips = self.i["x"].clone(), self.i["c"].clone(), self.i["skips"].clone()
        for j, e in enumerate(ends):
            for v in (x, c, skips):
                v[j, :, e:] = float("nan")
        return x, c, skips

    def check_items(self, what, x, c, skips, ends, x_out, s_out, s_tail=None):
        """Columns < e: the plain op on the item alone, bit for bit; columns >= e: untouched (the sentinel, or for a
        skip sum updated in place the input's own bits ``s_tail``)."""
        for j, e in enumerate(ends):
            assert bool((x_out[j, :, e:] == SENTINEL).all()), f"{what}: item {j} (ends at {e}): x_out written past its end"
            if s_tail is None:
                assert bool((s_out[j, :, e:] == SENTINEL).all()), f"{what}: item {j} (ends at {e}): skips_out written past its end"
            else:
                assert torch.equal(_bits(s_out[j, :, e:]), _bits(s_tail[j, :, e:])), f"{what}: item {j}: the skip tail changed"
            if e == 0:
                continue
            xa, sa = self.plain(x[j:j + 1, :, :e].contiguous(), c[j:j + 1, :, :e].contiguous(),
                                None if skips is None else skips[j:j + 1, :, :e].contiguous())
            assert not bool(torch.isnan(xa).any()) and not bool(torch.isnan(sa).any())
            for name, got, want in (("x_out", x_out[j, :, :e], xa[0]), ("skips_out", s_out[j, :, :e], sa[0])):
                assert torch.equal(_bits(got), _bits(want)), \
                    f"{what}: item {j} (ends at {e}): {name} differs from the item alone by {float((got - want).abs().max()):.3e}"


@pytest.mark.parametrize("dilation", [1, 4, 512])
@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_ragged_layer_is_every_item_alone(precision, dilation, device):
    for t, rate, frames, mode in LAUNCHES:
        what = f"{precision} d{dilation} T{t} rate{rate} frames{frames} skips {mode}"
        layer = Layer(precision, dilation, t, device)
        assert ops.wavenet_layer_ragged_supported(layer.desc(B, t), rate)
        ends = [min(f * rate, t) for f in frames]
        x, c, skips = layer.inputs_with_nan_tails(ends)
        table = torch.tensor(frames, dtype=torch.int32, device=device)
        gx = Sentinels((B, 64, t), device)
        gs = Sentinels((B, 64, t), device)
        if mode == "aliased":
            gs.out.copy_(skips)
            layer.ragged(x, c, gs.out, table, rate, skips_out=gs.out, x_out=gx.out)
            layer.check_items(what, x, c, skips, ends, gx.out, gs.out, s_tail=skips)
        else:
            s_in = skips if mode == "separate" else None
            layer.ragged(x, c, s_in, table, rate, skips_out=gs.out, x_out=gx.out)
            layer.check_items(what, x, c, s_in, ends, gx.out, gs.out)
        torch.cuda.synchronize()
        assert gx.guards_hold() and gs.guards_hold(), f"{what}: a store outside the tensors"


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_a_captured_ragged_launch_reads_the_table_of_the_moment(precision, device):
    t, rate, d = 1344, 4, 4
    layer = Layer(precision, d, t, device)
    x, c, skips = layer.i["x"], layer.i["c"], layer.i["skips"]
    table = torch.tensor((0, 1, 16, 17, 175), dtype=torch.int32, device=device)
    gx, gs = Sentinels((B, 64, t), device), Sentinels((B, 64, t), device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        layer.ragged(x, c, skips, table, rate, skips_out=gs.out, x_out=gx.out)  # (the LDS limit is set outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        layer.ragged(x, c, skips, table, rate, skips_out=gs.out, x_out=gx.out)
    other = (400, 175, 0, 17, 1)
    table.copy_(torch.tensor(other, dtype=torch.int32))
    gx.buf.fill_(SENTINEL)
    gs.buf.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    layer.check_items(f"{precision}: replay", x, c, skips, [min(f * rate, t) for f in other], gx.out, gs.out)
    assert gx.guards_hold() and gs.guards_hold()


@pytest.mark.parametrize("t", [1344, 1340])
@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_every_item_at_full_length_is_the_plain_batched_launch(precision, t, device):
    for d in (1, 512):
        layer = Layer(precision, d, t, device)
        x, c, skips = layer.i["x"], layer.i["c"], layer.i["skips"]
        full = torch.full((B,), (t + 3) // 4, dtype=torch.int32, device=device)
        for s_in in (skips, None):
            px, ps = layer.plain(x, c, s_in)
            rx, rs = layer.ragged(x, c, s_in, full, 4)
            assert torch.equal(_bits(px), _bits(rx)) and torch.equal(_bits(ps), _bits(rs)), f"{precision} d{d} T{t}"


# ---------------------------------------------------------------------------------------------------------- generator
FRAMES, T_PAD, W, UP = (0, 1, 3, 5, 9), 12, 2, 256
CONFIGS = {"one_stack": dict(PWG_G, layers=10, stacks=1),  # dilations 1 .. 512
           "three_stacks": dict(PWG_G, layers=6, stacks=3)}


def _generator(name, device):
    g = ParallelWaveGANGenerator(**CONFIGS[name])
    sd = synth_for(g, 11, synth.PWG_G_SCALE)
    g.load_state_dict(sd)
    return g.to(device).eval(), sd


@functools.lru_cache(maxsize=None)
def _items():
    """Per item its mel (T_j, 80) and noise (T_j * up,); the padded block the host builds and the padded noise."""
    feats = [synth.synth_input("c", (n, 80), seed=20 + j) for j, n in enumerate(FRAMES)]
    noises = [synth.synth_input("z", (n * UP,), seed=20 + j) for j, n in enumerate(FRAMES)]
    live = tuple(j for j, n in enumerate(FRAMES) if n > 0)
    group = RaggedGroup(live, tuple(FRAMES[j] for j in live), T_PAD)
    block = torch.zeros(len(FRAMES), T_PAD + 2 * W, 80)
    block[list(live)] = PWGRaggedSynthesizer.block_layout(group, feats, W, len(live), 80)
    c = block.transpose(1, 2).contiguous()
    z = torch.zeros(len(FRAMES), 1, T_PAD * UP)
    for j, n in enumerate(FRAMES):
        z[j, 0, :n * UP] = noises[j]
    return feats, noises, c, z


def _alone_inputs(j):
    _, noises, c, _ = _items()
    n = FRAMES[j]
    return noises[j].reshape(1, 1, -1), c[j:j + 1, :, :n + 2 * W].contiguous()


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The CPU oracle on every item alone, computed once."""
    g = ParallelWaveGANGenerator(**CONFIGS[name])
    sd = synth_for(g, 11, synth.PWG_G_SCALE)
    with torch.no_grad():
        return [None if n == 0 else torch_cpu.pwg_generator(sd, *_alone_inputs(j), **CONFIGS[name])
                for j, n in enumerate(FRAMES)]


def _table(frames, device):
    return torch.tensor(frames, dtype=torch.int32, device=device)


def _with_nan_tails(z, c):
    z, c = z.clone(), c.clone()
    for j, n in enumerate(FRAMES):
        z[j, :, n * UP:] = float("nan")
        c[j, :, n + 2 * W:] = float("nan")
    return z, c


@pytest.mark.parametrize("name", list(CONFIGS))
def test_generator_gives_every_item_what_it_gives_alone(name, device):
    g, _ = _generator(name, device)
    _, _, c, z = _items()
    c, z = c.to(device), z.to(device)
    c0, z0 = c.clone(), z.clone()
    with torch.no_grad():
        with ops.profile() as prof:
            y = g.forward_ragged(z, c, _table(FRAMES, device)).clone()
        assert prof.results["wavenet_layer_ragged_kernel"]["launches"] == CONFIGS[name]["layers"], sorted(prof.results)
        assert "wavenet_layer_kernel" not in prof.results and prof.results["zero_tail_kernel"]["launches"] == 4
        assert y.shape == (len(FRAMES), 1, T_PAD * UP)
        assert torch.equal(c, c0) and torch.equal(z, z0), "the caller's tensors were written"
        worst = 0.0
        for j, n in enumerate(FRAMES):
            if n == 0:
                continue
            za, ca = (v.to(device) for v in _alone_inputs(j))
            alone = g(za, ca)
            e_alone = max_abs(y[j:j + 1, :, :n * UP], alone)
            e_oracle = max_abs(y[j:j + 1, :, :n * UP], _oracle(name)[j])
            worst = max(worst, e_alone)
            print(f"{name} item {j} ({n} frames): |ragged - alone| {e_alone:.3e}  |ragged - oracle| {e_oracle:.3e}")
            assert e_alone <= ALONE_TOL, f"item {j}"
            assert e_oracle <= WAVE_TOL, f"item {j}"
        print(f"{name}: max |ragged - alone| over the items {worst:.3e}")
        # bitwise invariants, on the columns an item owns
        z_nan, c_nan = _with_nan_tails(z, c)
        y_nan = g.forward_ragged(z_nan, c_nan, _table(FRAMES, device))
        others = (4, 1, 2, 5, 9)
        y_others = g.forward_ragged(z, c, _table(others, device))
        for j, n in enumerate(FRAMES):
            assert torch.equal(_bits(y_nan[j, :, :n * UP]), _bits(y[j, :, :n * UP])), f"item {j}: NaN in the tails"
            if others[j] == n:
                assert torch.equal(_bits(y_others[j, :, :n * UP]), _bits(y[j, :, :n * UP])), \
                    f"item {j}: the other items' lengths changed its bits"


def test_generator_refuses_wrong_shapes_and_tables(device):
    g, _ = _generator("three_stacks", device)
    _, _, c, z = _items()
    c, z, table = c.to(device), z.to(device), _table(FRAMES, device)
    with pytest.raises(ValueError, match=r"expected \(B, 80, T_pad \+ 4\) features"):
        g.forward_ragged(z, c[0], table)
    with pytest.raises(ValueError, match=r"expected \(B, 80, T_pad \+ 4\) features"):
        g.forward_ragged(z, c[:, :40].contiguous(), table)
    with pytest.raises(ValueError, match=r"expected \(5, 1, 3072\) noise"):
        g.forward_ragged(z[:, :, :-256].contiguous(), c, table)
    with pytest.raises(ValueError, match=r"expected \(5, 1, 3072\) noise"):
        g.forward_ragged(z[:4], c, table)
    with pytest.raises(ValueError, match="frames table"):
        g.forward_ragged(z, c, table[:3])
    with pytest.raises(ValueError, match="frames table"):
        g.forward_ragged(z, c, torch.tensor(FRAMES, dtype=torch.int64, device=device))
    with pytest.raises(ValueError, match="frames table"):
        g.forward_ragged(z, c, torch.tensor(FRAMES, dtype=torch.int32))
    with pytest.raises(ValueError, match="frames table"):
        g.forward_ragged(z, c, list(FRAMES))


def test_generator_bf16(device):
    """bf16 operands: every item against the same item run alone in bf16, at the bar of
    tests/test_ragged_gpu.py::test_generator_bf16_on_tiny (error against error: twice the rms distance of the CPU bf16
    emulation from the fp32 oracle).  No sample of an item is left out."""
    name = "three_stacks"
    g, sd = _generator(name, device)
    _, _, c, z = _items()
    assert set_inference_precision(g, "bf16") > 0
    with torch.no_grad():
        with ops.profile() as prof:
            y = g.forward_ragged(z.to(device), c.to(device), _table(FRAMES, device)).clone()
        assert prof.results["wavenet_bf16_layer_ragged_kernel"]["launches"] == CONFIGS[name]["layers"], sorted(prof.results)
        assert "wavenet_layer_ragged_kernel" not in prof.results and "wavenet_bf16_layer_kernel" not in prof.results
        for j, n in enumerate(FRAMES):
            if n == 0:
                continue
            za, ca = _alone_inputs(j)
            alone = g(za.to(device), ca.to(device))
            with bf16_operands():
                emu = torch_cpu.pwg_generator(sd, za, ca, **CONFIGS[name])
            e, bar = rms((y[j:j + 1, :, :n * UP] - alone).cpu()), 2.0 * rms(emu - _oracle(name)[j])
            print(f"bf16 item {j} ({n} frames): rms(ragged - alone) {e:.3e}  bar {bar:.3e}")
            assert bar > 0 and e <= bar, f"item {j}"
            assert bool(torch.isfinite(y[j, :, :n * UP]).all())


# -------------------------------------------------------------------------------------------------------- synthesizer
def _feats(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return ([torch.randn(n, 80, generator=g) for n in lengths], [torch.randn(n * UP, generator=g) for n in lengths])


def test_synthesizer(device):
    g, _ = _generator("three_stacks", device)
    lengths, lengths2 = [10, 3, 20, 5, 16, 7, 2], [18, 6, 1, 24, 4, 8, 12]  # buckets 8 and 24, twice
    feats, noises = _feats(lengths, 1)
    synth_graph = PWGRaggedSynthesizer(g, max_batch=4, bucket_frames=8)
    eager = PWGRaggedSynthesizer(g, max_batch=4, bucket_frames=8, use_graph=False)
    assert synth_graph.max_frames == 32767 and synth_graph.context == 2
    assert [gr.t_pad for gr in synth_graph.plan(lengths).groups] == [8, 24]
    outs = synth_graph.synthesize_many(feats, noises=noises)
    assert synth_graph.captures == 2 and synth_graph.graphs_captured == 2
    with torch.no_grad():
        for n, f, x, y in zip(lengths, feats, noises, outs):
            assert y.shape == (n * UP,)
            e = max_abs(y, g.inference(f.to(device), x.reshape(-1, 1).to(device)).reshape(-1))
            print(f"{n} frames: |ragged - inference| {e:.3e}")
            assert e <= ALONE_TOL, "results out of input order, or wrong"
    feats2, noises2 = _feats(lengths2, 2)
    outs2 = synth_graph.synthesize_many(feats2, noises=noises2)
    assert synth_graph.captures == 2, "other lengths in the same buckets captured a new graph"
    for y, y_eager in zip(outs2, eager.synthesize_many(feats2, noises=noises2)):
        assert torch.equal(_bits(y), _bits(y_eager)), "a replay differs from the eager run"
    # PCM16 is the conversion of the float result
    for pcm, y in zip(synth_graph.synthesize_many_pcm16(feats2, noises=noises2), outs2):
        assert pcm.dtype == torch.int16 and torch.equal(pcm, to_pcm16(y))
    # noise drawn on the device: finite, of the right lengths, and not the same twice -- in graph and in eager mode
    for s in (synth_graph, eager):
        a, b = s.synthesize_many(feats2), s.synthesize_many(feats2)
        for n, ya, yb in zip(lengths2, a, b):
            assert ya.shape == (n * UP,) and bool(torch.isfinite(ya).all()) and not torch.equal(ya, yb)
    assert synth_graph.captures == 2, "drawn noise captured a new graph"
    # other weights are noticed: the graphs are captured again and give the new model's waveforms
    g.load_state_dict({k: v * 1.01 for k, v in g.state_dict().items()})
    outs3 = synth_graph.synthesize_many(feats2, noises=noises2)
    assert synth_graph.captures == 4
    with torch.no_grad():
        for f, x, y, y_old in zip(feats2, noises2, outs3, outs2):
            assert max_abs(y, g.inference(f.to(device), x.reshape(-1, 1).to(device)).reshape(-1)) <= ALONE_TOL
            assert not torch.equal(y, y_old)
    with pytest.raises(ValueError, match="item 1 is empty"):
        synth_graph.synthesize_many([feats[0], torch.zeros(0, 80)])
    with pytest.raises(ValueError, match=r"expected \(T, 80\)"):
        synth_graph.synthesize_many([torch.zeros(5, 79)])
    with pytest.raises(ValueError, match=r"item 0: expected \(2560,\) noise for 10 frames"):
        synth_graph.synthesize_many(feats[:1], noises=[noises[0][:-1]])
    with pytest.raises(ValueError, match="1 noises for 2 utterances"):
        synth_graph.synthesize_many(feats[:2], noises=noises[:1])


# --------------------------------------------------------------------------------------------------------------- CLI
def _checkpoint(tmp_path, cfg, name):
    import yaml

    d = tmp_path / name
    d.mkdir()
    model = ParallelWaveGANGenerator(**cfg)
    torch.save({"model": {"generator": synth_for(model, 11, synth.PWG_G_SCALE)}}, d / "checkpoint-1steps.pkl")
    with open(d / "config.yml", "w") as f:
        yaml.dump({"generator_type": "ParallelWaveGANGenerator", "generator_params": cfg, "format": "npy",
                   "sampling_rate": 22050}, f)
    return d / "checkpoint-1steps.pkl", model.upsample_factor


def test_cli_routes_a_pwg_checkpoint_through_the_ragged_synthesizer(tmp_path, monkeypatch, device):
    """``decode.main`` on tiny checkpoints: the non-causal one goes ``--batch-size`` utterances per forward through
    ``PWGRaggedSynthesizer`` (noise drawn on the device: the samples are not compared), the causal one keeps the loop
    over ``model.inference``; either way one WAV per utterance, of the right length and rate, and not silent."""
    import numpy as np

    import parallelwavegan_amd.utils as utils
    from parallelwavegan_amd.bin import decode

    calls = []

    class Spy(PWGRaggedSynthesizer):
        def synthesize_many_pcm16(self, feats, **kw):
            calls.append(len(feats))
            return super().synthesize_many_pcm16(feats, **kw)

    monkeypatch.setattr(utils, "PWGRaggedSynthesizer", Spy)
    dump = tmp_path / "dump"
    dump.mkdir()
    mels = {f"utt{j}": m.numpy() for j, m in enumerate(_feats([9, 2, 14], 7)[0])}
    for utt, mel in mels.items():
        np.save(dump / f"{utt}-feats.npy", mel)
    for name, cfg, expected_calls in (("plain", dict(CONFIGS["three_stacks"]), [2, 1]), ("causal", dict(synth.PWG_CAUSAL), [])):
        calls.clear()
        checkpoint, up = _checkpoint(tmp_path, cfg, name)
        out = tmp_path / f"wav_{name}"
        decode.main(["--dumpdir", str(dump), "--outdir", str(out), "--checkpoint", str(checkpoint), "--batch-size", "2",
                     "--verbose", "0"])
        assert calls == expected_calls, f"{name}: calls of PWGRaggedSynthesizer {calls}"
        assert sorted(p.name for p in out.iterdir()) == sorted(f"{utt}_gen.wav" for utt in mels)
        for utt, mel in mels.items():
            pcm, rate = decode.read_wav_pcm16(str(out / f"{utt}_gen.wav"))
            assert rate == 22050 and pcm.dtype == np.int16 and pcm.shape == (mel.shape[0] * up,), (name, utt)
            assert int(np.abs(pcm.astype(np.int32)).max()) > 100, f"{name} {utt}: a silent waveform"
