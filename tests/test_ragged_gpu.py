"""GPU: utterances of different lengths in one exact HiFi-GAN forward: ``ops.zero_tail``, the ragged
form of the split-operand residual unit, ``HiFiGANGenerator.forward_ragged``, ``utils.RaggedSynthesizer`` and the
``parallel-wavegan-decode`` command line.

The kernels are compared bit for bit: the ragged unit against ``ops.resunit_forward_split`` on every item alone, cropped
to the item's end, at the same MFMA shape.  The generator is compared per item against the CPU oracle (``WAVE_TOL``) and
against ``g.inference`` on the item alone (2e-5: one generator under two tile configurations, the bound of
tests/test_stream_gpu.py); everything past an item's end is an exact zero.  As in
tests/test_hifigan_resunit_split_gpu.py the admission tables are forced to "everything supported", so that the short test
inputs reach the unit kernel."""
import functools

import numpy as np
import pytest
import torch
import yaml

from oracle import torch_cpu
from parallelwavegan_amd import ops
from parallelwavegan_amd.bin import decode
from parallelwavegan_amd.layers.conv import _ConvNd
from parallelwavegan_amd.models import HiFiGANGenerator
from parallelwavegan_amd.utils import RaggedSynthesizer, set_inference_precision
from parallelwavegan_amd.utils.streaming import to_pcm16
from tests.bf16_emulation import bf16_operands, rms
from tests.golden import synth
from tests.test_conv_split_gpu import Guarded
from tests.util import WAVE_TOL, max_abs, synth_for

pytestmark = pytest.mark.gpu

ALONE_TOL = 2e-5  # one generator under two tile configurations (tests/test_stream_gpu.py)
UNIT_RAGGED, UNIT_PLAIN, ZERO_TAIL = "resunit_split_ragged_kernel", "resunit_split_kernel", "zero_tail_kernel"
SLOPE = 0.1


@pytest.fixture
def admit_all(monkeypatch):
    monkeypatch.setattr(_ConvNd, "split_exact", True)
    monkeypatch.setattr(_ConvNd, "split_admit_all", True)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _is_zero(t):
    """Exact +0.0f everywhere (not -0.0f, not NaN)."""
    return bool((_bits(t) == 0).all())


# ---------------------------------------------------------------------------------------------------------- zero_tail
GUARD = 16


def _zero_tail_case(shape, rate, frames, device, offset=0, run=None):
    """``zero_tail`` on a (B, C, T) view ``offset`` floats into a sentinel-guarded buffer whose tails hold NaN."""
    b, c, t = shape
    n = b * c * t
    g = torch.Generator().manual_seed(n + rate)
    head = torch.randn(shape, generator=g).to(device)
    buf = torch.full((GUARD + offset + n + GUARD,), 12345.0, device=device)
    y = buf[GUARD + offset:GUARD + offset + n].view(shape)
    y.copy_(head)
    ends = [min(f * rate, t) for f in frames]
    for i, e in enumerate(ends):
        y[i, :, e:] = float("nan")
    table = torch.tensor(frames, dtype=torch.int32, device=device)
    (run or (lambda y_, table_: ops.zero_tail(y_, table_, rate)))(y, table)
    torch.cuda.synchronize()
    assert bool((buf[:GUARD + offset] == 12345.0).all()) and bool((buf[GUARD + offset + n:] == 12345.0).all()), \
        "a store outside the tensor"
    for i, e in enumerate(ends):
        assert torch.equal(_bits(y[i, :, :e]), _bits(head[i, :, :e])), f"item {i}: the head changed"
        assert _is_zero(y[i, :, e:]), f"item {i}: the tail is not exact zeros"
    return y, table, ends


ZERO_TAIL_CASES = [((3, 5, 37), 1, (0, 17, 37)), ((2, 4, 64), 4, (3, 16))]


@pytest.mark.parametrize("shape,rate,frames", ZERO_TAIL_CASES)
@pytest.mark.parametrize("offset", [0, 1, 3])
def test_zero_tail(shape, rate, frames, offset, device):
    """Rows of odd T and a base that is only 4-B aligned take the scalar stores; NaN tails become exact zeros."""
    _zero_tail_case(shape, rate, frames, device, offset)


def test_zero_tail_spans_several_workgroups_and_clamps(device):
    """More than one column tile (1024 columns) and row group (8 rows); frames * rate past T is clamped to T."""
    _zero_tail_case((2, 19, 2501), 3, (1, 700), device, offset=1)
    _zero_tail_case((3, 9, 2048), 256, (4, 8, 9), device)


@pytest.mark.parametrize("shape,rate,frames", ZERO_TAIL_CASES)
def test_zero_tail_on_a_side_stream_and_captured(shape, rate, frames, device):
    side = torch.cuda.Stream()

    def on_side(y, table):
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.zero_tail(y, table, rate)
        torch.cuda.current_stream().wait_stream(side)

    _zero_tail_case(shape, rate, frames, device, run=on_side)
    # captured: the replay reads the table's values of the moment
    y, table, _ = _zero_tail_case(shape, rate, frames, device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.zero_tail(y, table, rate)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.zero_tail(y, table, rate)
    other = tuple(max(f - 1, 0) for f in frames)
    y.fill_(float("nan"))
    table.copy_(torch.tensor(other, dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    for i, f in enumerate(other):
        e = min(f * rate, shape[2])
        assert bool(torch.isnan(y[i, :, :e]).all()) and _is_zero(y[i, :, e:]), f"replay, item {i}"


# --------------------------------------------------------------------------------------------------- the ragged unit
UNIT_VARIANTS = [dict(bias=False, add2=False, out_div=1.0), dict(bias=True, add2=True, out_div=3.0),
                 dict(bias=True, add2=True, out_div=1.0), dict(bias=True, add2=False, out_div=3.0)]
UNIT_CASES = [(c, k, d, pair) for c in (32, 64) for k in (3, 7, 11) for d in (1, 5) for pair in (True, False)]


def _unit_geometry(c, k, pair):
    h = 256 if c == 32 else 128
    tile = ((h - (k - 1)) & ~3) if pair else h
    t = 3 * h + 40
    # items end at column 0, at 4, 4 before / at / 4 after a tile boundary, at T - 4 and at T
    return t, tile, (0, 4, tile - 4, tile, tile + 4, t - 4, t)


@functools.lru_cache(maxsize=None)
def _unit_inputs(c, k, t, b):
    g = torch.Generator().manual_seed(c * 1009 + k * 101 + t)
    return dict(x=torch.randn(b, c, t, generator=g), add2=torch.randn(b, c, t, generator=g),
                w1=torch.randn(c, c, k, generator=g) / (c * k) ** 0.5, w2=torch.randn(c, c, k, generator=g) / (c * k) ** 0.5,
                b1=torch.randn(c, generator=g), b2=torch.randn(c, generator=g))


@pytest.mark.parametrize("c,k,d,pair", UNIT_CASES, ids=["c%d_k%d_d%d_%s" % (c, k, d, "pair" if p else "single")
                                                        for c, k, d, p in UNIT_CASES])
def test_ragged_unit_is_every_item_alone(c, k, d, pair, device):
    t, tile, ends = _unit_geometry(c, k, pair)
    rate = 4
    b = len(ends)
    i = _unit_inputs(c, k, t, b)
    x, add2_full = i["x"].to(device), i["add2"].to(device)
    for j, e in enumerate(ends):  # the invariant: zero tails
        x[j, :, e:] = 0.0
        add2_full[j, :, e:] = 0.0
    wdesc = ops.make_conv_desc(1, c, c, 64, 64, k, pad_left=(k - 1) // 2)
    i1 = ops.pack_weight_split(wdesc, i["w1"].to(device))
    i2 = ops.pack_weight_split(wdesc, i["w2"].to(device)) if pair else None
    frames = torch.tensor([e // rate for e in ends], dtype=torch.int32, device=device)
    full = torch.full((b,), t // rate, dtype=torch.int32, device=device)
    for shape in (16, 32):
        for v in UNIT_VARIANTS:
            what = f"C{c} k{k} d{d} pair{pair} mfma {shape} {v}"
            b1 = i["b1"].to(device) if v["bias"] else None
            b2 = i["b2"].to(device) if (v["bias"] and pair) else None
            add2 = add2_full if v["add2"] else None
            desc = ops.make_resunit_desc(b, c, t, k, d, pair, SLOPE, SLOPE, v["out_div"])
            assert ops.resunit_split_ragged_supported(desc, rate)
            gd = Guarded((b, c, t), device)
            ops.resunit_forward_split_ragged(desc, x, frames, rate, i1, b1, i2, b2, add2, out=gd.out, mfma_shape=shape)
            y = gd.check(what)
            for j, e in enumerate(ends):
                assert _is_zero(y[j, :, e:]), f"{what}: item {j} (ends at {e}) is not exact zeros past its end"
                if e == 0:
                    continue
                alone = ops.resunit_forward_split(
                    ops.make_resunit_desc(1, c, e, k, d, pair, SLOPE, SLOPE, v["out_div"]), x[j:j + 1, :, :e].contiguous(),
                    i1, b1, i2, b2, None if add2 is None else add2[j:j + 1, :, :e].contiguous(), mfma_shape=shape)
                assert torch.equal(_bits(y[j, :, :e]), _bits(alone[0])), \
                    f"{what}: item {j} (ends at {e}, tile {tile}) differs from the item alone by " \
                    f"{float((y[j, :, :e] - alone[0]).abs().max()):.3e}"
            # every item at T: the plain kernel's bits (on inputs without zero tails)
            xf = i["x"].to(device)
            af = i["add2"].to(device) if v["add2"] else None
            plain = ops.resunit_forward_split(desc, xf, i1, b1, i2, b2, af, mfma_shape=shape)
            ragged = ops.resunit_forward_split_ragged(desc, xf, full, rate, i1, b1, i2, b2, af, mfma_shape=shape)
            assert torch.equal(_bits(plain), _bits(ragged)), f"{what}: all items at T differ from the plain kernel"


# --------------------------------------------------------------------------------------------------------- generator
B, T_MAX, FRAMES = 4, 24, (24, 17, 5, 1)
# tiny_odd: the 32-channel stage sits at rate 3, where the ragged unit is not covered (rate % 4): the unit's defining chain
CONFIGS = {"v1": synth.HIFIGAN_V1, "tiny": synth.HIFIGAN_TINY,
           "tiny_odd": dict(synth.HIFIGAN_TINY, upsample_scales=[3, 2, 2], upsample_kernel_sizes=[6, 4, 4])}
CONV_SPLIT = "conv1d_split_mfma_kernel"


def _generator(name, device):
    g = HiFiGANGenerator(**CONFIGS[name])
    sd = synth_for(g, 11, 1.25)
    g.load_state_dict(sd)
    g.remove_weight_norm()
    return g.to(device).eval(), sd


@functools.lru_cache(maxsize=None)
def _mel(name):
    return synth.synth_input("c", (B, 80, T_MAX), seed=T_MAX)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The CPU oracle on every item alone, computed once."""
    g = HiFiGANGenerator(**CONFIGS[name])
    sd = synth_for(g, 11, 1.25)
    with torch.no_grad():
        return [torch_cpu.hifigan_generator(sd, _mel(name)[j:j + 1, :, :n].contiguous(), **CONFIGS[name])
                for j, n in enumerate(FRAMES)]


def _table(frames, device):
    return torch.tensor(frames, dtype=torch.int32, device=device)


@pytest.mark.parametrize("name", ["v1", "tiny", "tiny_odd"])
def test_generator_gives_every_item_what_it_gives_alone(name, admit_all, device):
    g, _ = _generator(name, device)
    up = g.upsample_factor
    c = _mel(name).to(device)
    c_zero = c.clone()
    for j, n in enumerate(FRAMES):
        c_zero[j, :, n:] = 0.0
    with torch.no_grad():
        with ops.profile() as prof:
            y = g.forward_ragged(c, _table(FRAMES, device)).clone()
        assert ZERO_TAIL in prof.results and UNIT_PLAIN not in prof.results, sorted(prof.results)
        if name == "tiny_odd":  # 4 units of two convolutions each as their chain of split launches
            assert UNIT_RAGGED not in prof.results and prof.results[CONV_SPLIT]["launches"] >= 8, prof.results
        else:
            # V1: 2 stages x 3 kernel sizes x 3 dilations (rates 128 and 256); TINY: its 32-channel stage (rate 4) only
            assert prof.results[UNIT_RAGGED]["launches"] == (18 if name == "v1" else 4), prof.results[UNIT_RAGGED]
        assert y.shape == (B, 1, T_MAX * up)
        alone = [g(c[j:j + 1, :, :n].contiguous()).clone() for j, n in enumerate(FRAMES)]
        plain = g(c_zero).clone()
        for j, (n, ref) in enumerate(zip(FRAMES, _oracle(name))):
            e_oracle, e_alone = max_abs(y[j:j + 1, :, :n * up], ref), max_abs(y[j:j + 1, :, :n * up], alone[j])
            print(f"{name} item {j} ({n} frames): |ragged - oracle| {e_oracle:.3e}  |ragged - alone| {e_alone:.3e}  "
                  f"|plain padded forward - alone| {max_abs(plain[j:j + 1, :, :n * up], alone[j]):.3e}")
            assert e_oracle <= WAVE_TOL, f"item {j}"
            if name == "v1":
                assert e_alone <= ALONE_TOL, f"item {j}"
            assert _is_zero(y[j, :, n * up:]), f"item {j}: not exact zeros past its end"
        # the control: zero mel frames are not what an item sees alone (a hidden layer is not zero where the mel is)
        assert max_abs(plain[2:3, :, :FRAMES[2] * up], alone[2]) > 1e-3
        # bitwise invariants
        c_nan = c.clone()
        for j, n in enumerate(FRAMES):
            c_nan[j, :, n:] = float("nan")
        assert torch.equal(_bits(g.forward_ragged(c_nan, _table(FRAMES, device))), _bits(y)), "NaN in the mel tails"
        others = (3, 17, 24, 9)
        y2 = g.forward_ragged(c, _table(others, device))
        assert torch.equal(_bits(y2[1]), _bits(y[1])), "the other items' lengths changed bits of an item"
        y3 = g.forward_ragged(c_nan, _table((24, 0, 5, 1), device))
        assert _is_zero(y3[1]), "an unused item is not all zeros"
        assert torch.equal(_bits(y3[0]), _bits(y[0])) and torch.equal(_bits(y3[2:]), _bits(y[2:]))


def test_generator_bf16_on_tiny(admit_all, device):
    """bf16 operands: every item against the same item run alone in bf16, at the bar of tests/test_hifigan_bf16_gpu.py
    (error against error: twice the rms distance of the CPU bf16 emulation from the fp32 oracle)."""
    g, _ = _generator("tiny", device)
    sd = synth_for(HiFiGANGenerator(**synth.HIFIGAN_TINY), 11, 1.25)
    up = g.upsample_factor
    c = _mel("tiny").to(device)
    assert set_inference_precision(g, "bf16") > 0
    with torch.no_grad():
        y = g.forward_ragged(c, _table(FRAMES, device)).clone()
        for j, (n, ref) in enumerate(zip(FRAMES, _oracle("tiny"))):
            alone = g(c[j:j + 1, :, :n].contiguous())
            with bf16_operands():
                emu = torch_cpu.hifigan_generator(sd, _mel("tiny")[j:j + 1, :, :n].contiguous(), **synth.HIFIGAN_TINY)
            e, bar = rms((y[j:j + 1, :, :n * up] - alone).cpu()), 2.0 * rms(emu - ref)
            print(f"tiny bf16 item {j} ({n} frames): rms(ragged - alone) {e:.3e}  bar {bar:.3e}")
            assert bar > 0 and e <= bar, f"item {j}"
            assert _is_zero(y[j, :, n * up:])


# ------------------------------------------------------------------------------------------------------- synthesizer
def _feats(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, 80, generator=g) for n in lengths]


def test_synthesizer(admit_all, device):
    g, _ = _generator("tiny", device)
    lengths, lengths2 = [40, 3, 90, 20, 64, 31, 10], [70, 25, 5, 96, 12, 30, 50]  # buckets 32 and 96, twice
    feats = _feats(lengths, 1)
    synth_graph = RaggedSynthesizer(g, max_batch=4, bucket_frames=32)
    eager = RaggedSynthesizer(g, max_batch=4, bucket_frames=32, use_graph=False)
    assert [gr.t_pad for gr in synth_graph.plan(lengths).groups] == [32, 96]
    outs = synth_graph.synthesize_many(feats)
    assert synth_graph.captures == 2 and synth_graph.graphs_captured == 2
    for n, f, y in zip(lengths, feats, outs):
        assert y.shape == (n * g.upsample_factor,)
        e = max_abs(y, g.inference(f.to(device)).reshape(-1))
        print(f"{n} frames: |ragged - inference| {e:.3e}")
        assert e <= ALONE_TOL, "results out of input order, or wrong"
    feats2 = _feats(lengths2, 2)
    outs2 = synth_graph.synthesize_many(feats2)
    assert synth_graph.captures == 2, "other lengths in the same buckets captured a new graph"
    for y, y_eager in zip(outs2, eager.synthesize_many(feats2)):
        assert torch.equal(_bits(y), _bits(y_eager)), "a replay differs from the eager run"
    # PCM16 is the conversion of the float result
    for pcm, y in zip(synth_graph.synthesize_many_pcm16(feats2), outs2):
        assert pcm.dtype == torch.int16 and torch.equal(pcm, to_pcm16(y))
    # other weights are noticed: the graphs are captured again and give the new model's waveforms
    g.load_state_dict({k: v * 1.01 for k, v in g.state_dict().items()})
    outs3 = synth_graph.synthesize_many(feats2)
    assert synth_graph.captures == 4
    for f, y, y_old in zip(feats2, outs3, outs2):
        assert max_abs(y, g.inference(f.to(device)).reshape(-1)) <= ALONE_TOL
        assert not torch.equal(y, y_old)
    with pytest.raises(ValueError, match="item 1 is empty"):
        synth_graph.synthesize_many([feats[0], torch.zeros(0, 80)])
    with pytest.raises(ValueError, match=r"expected \(T, 80\)"):
        synth_graph.synthesize_many([torch.zeros(5, 79)])


# --------------------------------------------------------------------------------------------------------------- CLI
def test_cli_writes_what_inference_gives(admit_all, tmp_path, device):
    """``decode.main`` on a TINY checkpoint: the WAV files hold ``to_pcm16(model.inference(c))`` to within 1 LSB.  The
    ragged batch and the utterance alone differ by fp32 summation order (<= 2e-5 of full scale), which moves a sample
    across a rounding boundary only where it lies that close to one.  Measured on an MI355X: 0 of 1584 samples differ
    (0.000 %; the figure is printed, the bar is 1 %)."""
    cfg = dict(synth.HIFIGAN_TINY)
    model = HiFiGANGenerator(**cfg)
    sd = synth_for(model, 11, 1.25)
    model.load_state_dict(sd)
    torch.save({"model": {"generator": sd}}, tmp_path / "checkpoint-1steps.pkl")
    with open(tmp_path / "config.yml", "w") as f:
        yaml.dump({"generator_type": "HiFiGANGenerator", "generator_params": {k: (list(v) if isinstance(v, tuple) else v)
                                                                              for k, v in cfg.items()},
                   "format": "npy", "sampling_rate": 22050}, f)
    dump = tmp_path / "dump"
    dump.mkdir()
    mels = {f"utt{j}": m.numpy() for j, m in enumerate(_feats([37, 8, 21], 7))}
    for utt, mel in mels.items():
        np.save(dump / f"{utt}-feats.npy", mel)
    # the inputs are not pathological: on the CPU oracle no mass of samples sits on a rounding boundary (a uniform
    # fractional part puts 4e-5 of the samples within 2e-5 LSB of one)
    with torch.no_grad():
        for utt, mel in mels.items():
            ref = torch_cpu.hifigan_generator(sd, torch.from_numpy(mel.T.copy()).unsqueeze(0), **cfg).reshape(-1).double()
            frac = (ref.clamp(-1, 1) * 32767 - 0.5).frac().abs()  # 0 on a boundary
            assert float((torch.minimum(frac, 1 - frac) < 2e-5).double().mean()) < 1e-3, utt
            assert float(ref.abs().max()) > 1e-2, "a silent waveform would test nothing"
    decode.main(["--dumpdir", str(dump), "--outdir", str(tmp_path / "wav"), "--checkpoint",
                 str(tmp_path / "checkpoint-1steps.pkl"), "--batch-size", "2", "--verbose", "0"])
    model.remove_weight_norm()
    model = model.to(device).eval()
    differ = total = 0
    for utt, mel in mels.items():
        pcm, rate = decode.read_wav_pcm16(str(tmp_path / "wav" / f"{utt}_gen.wav"))
        with torch.no_grad():
            want = to_pcm16(model.inference(torch.from_numpy(mel).to(device)).reshape(-1)).cpu().numpy()
        assert rate == 22050 and pcm.shape == want.shape == (mel.shape[0] * model.upsample_factor,)
        delta = np.abs(pcm.astype(np.int32) - want.astype(np.int32))
        assert delta.max() <= 1, f"{utt}: {delta.max()} LSB"
        differ, total = differ + int((delta != 0).sum()), total + delta.size
    print(f"samples that differ by 1 LSB: {differ} of {total} ({100.0 * differ / total:.3f} %)")
    assert differ / total < 0.01
