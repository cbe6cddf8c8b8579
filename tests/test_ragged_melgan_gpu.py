"""GPU: utterances of different lengths in one exact (multi-band) MelGAN forward: ``ops.mirror_tail``,
the ragged form of the one-launch residual stack, ``MelGANGenerator.forward_ragged``, ``utils.MelGANRaggedSynthesizer``
and the ``parallel-wavegan-decode`` command line on a MelGAN checkpoint.

The kernels are compared bit for bit: ``mirror_tail`` against the columns it mirrors, the ragged stack against
``ops.resstack_forward`` on every item alone, cropped to the item's end (an end below 64 columns, which the plain kernel
does not take, against a float64 CPU evaluation at the bound of tests/test_resstack_gpu.py).  The generator is compared
per item against the CPU oracle (``WAVE_TOL``) and against ``g`` on the item alone (2e-5: one generator under two tile
configurations, the bound of tests/test_ragged_gpu.py); everything past an item's end is an exact zero."""
import functools

import numpy as np
import pytest
import torch
import yaml

from oracle import torch_cpu
from parallelwavegan_amd import layers, ops
from parallelwavegan_amd.bin import decode
from parallelwavegan_amd.models import MelGANGenerator
from parallelwavegan_amd.utils import MelGANRaggedSynthesizer
from parallelwavegan_amd.utils.streaming import to_pcm16
from tests.golden import synth
from tests.test_conv_split_gpu import Guarded
from tests.test_ragged_gpu import ALONE_TOL, GUARD, ZERO_TAIL_CASES, _bits, _is_zero, _table
from tests.test_resstack_gpu import _reference
from tests.test_stream_melgan_lookahead_gpu import MB_G, TINY, TINY_MB
from tests.util import WAVE_TOL, max_abs, synth_for

pytestmark = pytest.mark.gpu

STACK_RAGGED, STACK_PLAIN, MIRROR_TAIL = "resstack_ragged_kernel", "resstack_kernel", "mirror_tail_kernel"
SLOPE = 0.2


# -------------------------------------------------------------------------------------------------------- mirror_tail
def _mirror_tail_case(shape, rate, frames, pad, device, offset=0, run=None, check_mirror=True):
    """``mirror_tail`` on a (B, C, T) view ``offset`` floats into a sentinel-guarded buffer whose tails hold NaN."""
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
    (run or (lambda y_, table_: ops.mirror_tail(y_, table_, rate, pad)))(y, table)
    torch.cuda.synchronize()
    assert bool((buf[:GUARD + offset] == 12345.0).all()) and bool((buf[GUARD + offset + n:] == 12345.0).all()), \
        "a store outside the tensor"
    for i, e in enumerate(ends):
        assert torch.equal(_bits(y[i, :, :e]), _bits(head[i, :, :e])), f"item {i}: the head changed"
        m = min(pad, t - e) if e > 0 else 0  # mirror columns inside the buffer
        if check_mirror and m:
            assert e - 1 - m >= 0, "a test case whose reflection is undefined"
            want = head[i, :, e - 1 - m:e - 1].flip(-1)  # column e + j holds column e - 2 - j
            assert torch.equal(_bits(y[i, :, e:e + m]), _bits(want)), f"item {i}: the mirror columns"
        assert _is_zero(y[i, :, e + m:]), f"item {i}: not exact zeros behind the mirror"
    return buf, y, table, ends


@pytest.mark.parametrize("shape,rate,frames", ZERO_TAIL_CASES + [((3, 5, 37), 1, (12, 33, 36))])
@pytest.mark.parametrize("offset", [0, 1, 3])
def test_mirror_tail(shape, rate, frames, offset, device):
    """Rows of odd T and a base that is only 4-B aligned; a mirror cut off by the row's end; NaN tails; and pad = 0 is
    ``zero_tail`` bit for bit."""
    for pad in (0, 1, 3, 9):
        buf, _, _, _ = _mirror_tail_case(shape, rate, frames, pad, device, offset)
        if pad == 0:
            zt, _, _, _ = _mirror_tail_case(shape, rate, frames, 0, device, offset,
                                            run=lambda y, table: ops.zero_tail(y, table, rate))
            assert torch.equal(_bits(buf), _bits(zt)), "pad = 0 is not zero_tail"


def test_mirror_tail_spans_several_workgroups(device):
    """More than one column tile (1024 columns) and row group (8 rows), a mirror across a tile boundary (item 1 ends at
    column 2043 of its shifted rows), frames * rate past T clamped to T."""
    _mirror_tail_case((2, 19, 2501), 3, (40, 681), 27, device, offset=1)
    _mirror_tail_case((2, 19, 2501), 3, (341, 900), 27, device, offset=1)


def test_mirror_tail_of_an_item_not_longer_than_pad_stays_inside(device):
    """``e <= pad``: reflection is undefined, the mirror values are unspecified, and nothing is stored or read outside."""
    _mirror_tail_case((3, 3, 40), 1, (1, 2, 9), 9, device, offset=1, check_mirror=False)
    _mirror_tail_case((2, 3, 8), 1, (1, 5), 9, device, check_mirror=False)


def test_mirror_tail_on_a_side_stream_and_captured(device):
    shape, rate, frames, pad = (2, 4, 64), 4, (5, 14), 3
    side = torch.cuda.Stream()

    def on_side(y, table):
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.mirror_tail(y, table, rate, pad)
        torch.cuda.current_stream().wait_stream(side)

    _mirror_tail_case(shape, rate, frames, pad, device, run=on_side)
    # captured: the replay reads the table's values of the moment
    _, y, table, _ = _mirror_tail_case(shape, rate, frames, pad, device)
    on_side(y, table)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.mirror_tail(y, table, rate, pad)
    other = (4, 13)
    head = torch.randn(shape, generator=torch.Generator().manual_seed(3)).to(device)
    y.copy_(head)
    table.copy_(torch.tensor(other, dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    for i, f in enumerate(other):
        e = f * rate
        assert torch.equal(_bits(y[i, :, :e]), _bits(head[i, :, :e]))
        assert torch.equal(_bits(y[i, :, e:e + pad]), _bits(head[i, :, e - 1 - pad:e - 1].flip(-1))), f"replay, item {i}"
        assert _is_zero(y[i, :, e + pad:]), f"replay, item {i}"


# --------------------------------------------------------------------------------------------------- the ragged stack
STACK_N = {48: 192, 96: 128, 192: 64}  # output columns per workgroup (csrc/resstack.hip)
STACK_RATE = 4


@functools.lru_cache(maxsize=None)
def _stack_inputs(c, t, b):
    g = torch.Generator().manual_seed(c * 1009 + t)
    return dict(x=torch.randn(b, c, t, generator=g), w1=torch.randn(c, c, 3, generator=g) / (3 * c) ** 0.5,
                w2=torch.randn(c, c, 1, generator=g) / c ** 0.5, ws=torch.randn(c, c, 1, generator=g) / c ** 0.5,
                b1=torch.randn(c, generator=g), b2=torch.randn(c, generator=g), bs=torch.randn(c, generator=g))


def _against_float64(y, x, i, bias, d, what):
    """An end the plain kernel does not take (fewer than 64 columns): the bound of tests/test_resstack_gpu.py."""
    want, _ = _reference(x, i["w1"], bias[0], i["w2"], bias[1], i["ws"], bias[2], d, SLOPE)
    err = (y.cpu().double() - want).abs().max().item() / want.abs().max().item()
    print(f"{what}: relative error against float64 {err:.3e}")
    assert err <= 3e-6, what


@pytest.mark.parametrize("c", [48, 96, 192])
@pytest.mark.parametrize("d", [1, 9, 27])
def test_ragged_stack_is_every_item_alone(c, d, device):
    n = STACK_N[c]
    t = 3 * n + 40
    # items end at column 0, at 64, 4 before / at / 4 after a tile boundary, at T - 4 and at T; and at 32 (d < 32)
    ends = (0, 64, n - 4, n, n + 4, t - 4, t) + ((32,) if d < 27 else ())
    b = len(ends)
    i = _stack_inputs(c, t, b)
    x = i["x"].to(device)
    x_nan = x.clone()
    for j, e in enumerate(ends):
        x_nan[j, :, e:] = float("nan")
    img = ops.resstack_pack_weight(i["w1"].to(device), None, i["w2"].to(device), None, i["ws"].to(device), None)
    frames = _table([e // STACK_RATE for e in ends], device)
    full = _table([t // STACK_RATE] * b, device)
    assert ops.resstack_ragged_supported(c, t, d, STACK_RATE)
    for with_bias in (True, False):
        what = f"C{c} d{d} bias{with_bias}"
        bias_cpu = [i[k] if with_bias else None for k in ("b1", "b2", "bs")]
        bias = [None if v is None else v.to(device) for v in bias_cpu]
        gd = Guarded((b, c, t), device)
        with ops.profile() as prof:
            ops.resstack_forward_ragged(x_nan, frames, STACK_RATE, img, d, SLOPE, *bias, out=gd.out)
        assert prof.results[STACK_RAGGED]["launches"] == 1 and STACK_PLAIN not in prof.results
        y = gd.check(what)
        for j, e in enumerate(ends):
            assert _is_zero(y[j, :, e:]), f"{what}: item {j} (ends at {e}) is not exact zeros past its end"
            if e == 0:
                continue
            if e < 64:  # the plain kernel does not take it (t < 64)
                assert not ops.resstack_supported(c, e, d)
                _against_float64(y[j:j + 1, :, :e], x[j:j + 1, :, :e], i, bias_cpu, d, f"{what} item {j} (ends at {e})")
                continue
            alone, _ = ops.resstack_forward(x[j:j + 1, :, :e].contiguous(), img, d, SLOPE, *bias)
            assert torch.equal(_bits(y[j, :, :e]), _bits(alone[0])), \
                f"{what}: item {j} (ends at {e}, tile {n}) differs from the item alone by " \
                f"{float((y[j, :, :e] - alone[0]).abs().max()):.3e}"
        # every item at T: the plain kernel's bits
        plain, _ = ops.resstack_forward(x, img, d, SLOPE, *bias)
        ragged = ops.resstack_forward_ragged(x, full, STACK_RATE, img, d, SLOPE, *bias)
        assert torch.equal(_bits(plain), _bits(ragged)), f"{what}: all items at T differ from the plain kernel"


# --------------------------------------------------------------------------------------------------------- generator
B, T_MAX, FRAMES = 4, 24, (24, 17, 5, 4)
CONFIGS = {"mb": MB_G,        # fused stacks at rates 8, 32 and 64
           "tiny_mb": TINY_MB,  # odd rates: the three-launch path
           "tiny": TINY}      # a small plain MelGAN: channels 64, scales [4, 2, 2], two stacks
SEED = 21


def _state(name):
    return synth_for(MelGANGenerator(**CONFIGS[name]), SEED, synth.MELGAN_G_SCALE)


def _generator(name, device):
    g = MelGANGenerator(**CONFIGS[name])
    g.load_state_dict(_state(name))
    g.remove_weight_norm()
    return g.to(device).eval()


@functools.lru_cache(maxsize=None)
def _mel():
    return synth.synth_input("c", (B, 80, T_MAX), seed=T_MAX)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The CPU oracle on every item alone, computed once."""
    sd = _state(name)
    with torch.no_grad():
        return [torch_cpu.melgan_generator(sd, _mel()[j:j + 1, :, :n].contiguous(), **CONFIGS[name])
                for j, n in enumerate(FRAMES)]


@pytest.mark.parametrize("name", ["mb", "tiny_mb", "tiny"])
def test_generator_gives_every_item_what_it_gives_alone(name, device):
    g = _generator(name, device)
    up = g.upsample_factor
    assert g.ragged_min_frames == 4 and g.ragged_slack_frames == 3
    assert all(n in (0, T_MAX) or 4 <= n <= T_MAX - 3 for n in FRAMES)
    c = _mel().to(device)
    c_zero = c.clone()
    for j, n in enumerate(FRAMES):
        c_zero[j, :, n:] = 0.0
    with torch.no_grad():
        c_before = c.clone()
        with ops.profile() as prof:
            y = g.forward_ragged(c, _table(FRAMES, device)).clone()
        assert torch.equal(c, c_before), "the caller's features were written"
        assert STACK_PLAIN not in prof.results, sorted(prof.results)
        if name == "mb":  # 3 stages x 4 stacks, one launch each; the mel copy, behind the first convolution, behind the
            # last stack, behind the last convolution
            assert prof.results[STACK_RAGGED]["launches"] == 12, prof.results[STACK_RAGGED]
            assert prof.results[MIRROR_TAIL]["launches"] <= 4, prof.results[MIRROR_TAIL]
        else:
            assert STACK_RAGGED not in prof.results and MIRROR_TAIL in prof.results
        assert y.shape == (B, CONFIGS[name]["out_channels"], T_MAX * up)
        alone = [g(c[j:j + 1, :, :n].contiguous()).clone() for j, n in enumerate(FRAMES)]
        plain = g(c_zero).clone()
        for j, (n, ref) in enumerate(zip(FRAMES, _oracle(name))):
            e_oracle, e_alone = max_abs(y[j:j + 1, :, :n * up], ref), max_abs(y[j:j + 1, :, :n * up], alone[j])
            print(f"{name} item {j} ({n} frames): |ragged - oracle| {e_oracle:.3e}  |ragged - alone| {e_alone:.3e}  "
                  f"|plain padded forward - alone| {max_abs(plain[j:j + 1, :, :n * up], alone[j]):.3e}")
            assert e_oracle <= WAVE_TOL, f"item {j}"
            assert e_alone <= ALONE_TOL, f"item {j}"
            assert _is_zero(y[j, :, n * up:]), f"item {j}: not exact zeros past its end"
        # the control: zero mel frames are not what an item sees alone (no reflection at its end, and a hidden layer is
        # not zero where the mel is)
        assert max_abs(plain[2:3, :, :FRAMES[2] * up], alone[2]) > 1e-3
        # bitwise invariants
        c_nan = c.clone()
        for j, n in enumerate(FRAMES):
            c_nan[j, :, n:] = float("nan")
        assert torch.equal(_bits(g.forward_ragged(c_nan, _table(FRAMES, device))), _bits(y)), "NaN in the mel tails"
        others = (4, 17, 24, 9)
        y2 = g.forward_ragged(c, _table(others, device))
        assert torch.equal(_bits(y2[1]), _bits(y[1])), "the other items' lengths changed bits of an item"
        y3 = g.forward_ragged(c_nan, _table((24, 0, 5, 4), device))
        assert _is_zero(y3[1]), "an unused item is not all zeros"
        assert torch.equal(_bits(y3[0]), _bits(y[0])) and torch.equal(_bits(y3[2:]), _bits(y[2:]))


def test_generator_refuses_wrong_shapes_and_tables(device):
    g = _generator("tiny", device)
    c = _mel().to(device)
    with pytest.raises(ValueError, match=r"expected \(B, in_channels, T_max\)"):
        g.forward_ragged(c[0], _table(FRAMES, device))
    with pytest.raises(RuntimeError, match="frames table"):
        g.forward_ragged(c, _table(FRAMES[:3], device))
    with pytest.raises(RuntimeError, match="frames table"):
        g.forward_ragged(c, torch.tensor(FRAMES, dtype=torch.int64, device=device))


# ------------------------------------------------------------------------------------------------------- synthesizer
def _feats(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, 80, generator=g) for n in lengths]


def _mb_waveform_oracle(sd, cfg, feat):
    """The CPU oracle's waveform of one utterance: its sub-bands through the oracle's PQMF synthesis."""
    with torch.no_grad():
        sub = torch_cpu.melgan_generator(sd, feat.t().unsqueeze(0).contiguous(), **cfg)
        return torch_cpu.pqmf_synthesis(sub, subbands=cfg["out_channels"]).reshape(-1)


def test_synthesizer(device):
    g = _generator("tiny_mb", device)
    g.pqmf = layers.PQMF(subbands=4).to(device)
    sd = _state("tiny_mb")
    k = g.upsample_factor * 4
    # with the slack of 3 frames: buckets 32 (29 + 3) and 96 (90 + 3, 93 + 3), twice
    lengths, lengths2 = [40, 4, 90, 20, 61, 29, 10], [70, 25, 5, 93, 12, 29, 50]
    feats = _feats(lengths, 1)
    synth_graph = MelGANRaggedSynthesizer(g, max_batch=4, bucket_frames=32)
    eager = MelGANRaggedSynthesizer(g, max_batch=4, bucket_frames=32, use_graph=False)
    assert (synth_graph.min_frames, synth_graph.slack_frames, synth_graph.up) == (4, 3, k)
    assert [gr.t_pad for gr in synth_graph.plan(lengths).groups] == [32, 96]
    assert [gr.t_pad for gr in synth_graph.plan(lengths2).groups] == [32, 96]
    outs = synth_graph.synthesize_many(feats)
    assert synth_graph.captures == 2 and synth_graph.graphs_captured == 2
    for n, f, y in zip(lengths, feats, outs):
        assert y.shape == (n * k,)
        e = max_abs(y, g.inference(f.to(device)).reshape(-1))
        e_oracle = max_abs(y, _mb_waveform_oracle(sd, TINY_MB, f))
        print(f"{n} frames: |ragged - inference| {e:.3e}  |ragged - oracle| {e_oracle:.3e}")
        assert e <= ALONE_TOL, "results out of input order, or wrong"
        assert e_oracle <= WAVE_TOL
    feats2 = _feats(lengths2, 2)
    outs2 = synth_graph.synthesize_many(feats2)
    assert synth_graph.captures == 2, "other lengths in the same buckets captured a new graph"
    for y, y_eager in zip(outs2, eager.synthesize_many(feats2)):
        assert torch.equal(_bits(y), _bits(y_eager)), "a replay differs from the eager run"
    # PCM16 is the conversion of the float result
    for pcm, y in zip(synth_graph.synthesize_many_pcm16(feats2), outs2):
        assert pcm.dtype == torch.int16 and torch.equal(pcm, to_pcm16(y))
    # other weights are noticed: the graphs are captured again and give the new model's waveforms
    g.load_state_dict({k_: v * 1.01 for k_, v in g.state_dict().items() if not k_.startswith("pqmf.")}, strict=False)
    outs3 = synth_graph.synthesize_many(feats2)
    assert synth_graph.captures == 4
    for f, y, y_old in zip(feats2, outs3, outs2):
        assert max_abs(y, g.inference(f.to(device)).reshape(-1)) <= ALONE_TOL
        assert not torch.equal(y, y_old)
    with pytest.raises(ValueError, match="item 1 has 3 frames, fewer than reflection can pad"):
        synth_graph.synthesize_many([feats[0], torch.zeros(3, 80)])
    with pytest.raises(ValueError, match=r"expected \(T, 80\)"):
        synth_graph.synthesize_many([torch.zeros(5, 79)])


# --------------------------------------------------------------------------------------------------------------- CLI
CLI_LENGTHS, CLI_SEED = [37, 8, 21], 7


def test_cli_writes_what_inference_gives(tmp_path, device):
    """``decode.main`` on a tiny multi-band checkpoint: the WAV files hold ``to_pcm16(model.inference(c))`` to within 1
    LSB.  The ragged batch and the utterance alone differ by fp32 summation order (<= 2e-5 of full scale), which moves a
    sample across a rounding boundary only where it lies that close to one; the fraction that differ is printed, the bar
    is 1 %.  Measured on an MI355X: 7 of 1584 samples differ (0.442 %)."""
    cfg = dict(TINY_MB)
    model = MelGANGenerator(**cfg)
    sd = _state("tiny_mb")
    model.load_state_dict(sd)
    torch.save({"model": {"generator": sd}}, tmp_path / "checkpoint-1steps.pkl")
    with open(tmp_path / "config.yml", "w") as f:
        yaml.dump({"generator_type": "MelGANGenerator", "generator_params": cfg, "format": "npy", "sampling_rate": 24000},
                  f)
    dump = tmp_path / "dump"
    dump.mkdir()
    mels = {f"utt{j}": m.numpy() for j, m in enumerate(_feats(CLI_LENGTHS, CLI_SEED))}
    for utt, mel in mels.items():
        np.save(dump / f"{utt}-feats.npy", mel)
    # the inputs are not pathological: on the CPU oracle the waveforms are not silent and no mass of samples sits on a
    # rounding boundary (a uniform fractional part puts 4e-5 of the samples within 2e-5 LSB of one)
    for utt, mel in mels.items():
        ref = _mb_waveform_oracle(sd, cfg, torch.from_numpy(mel)).double()
        frac = (ref.clamp(-1, 1) * 32767 - 0.5).frac().abs()  # 0 on a boundary
        assert float((torch.minimum(frac, 1 - frac) < 2e-5).double().mean()) < 1e-3, utt
        assert float(ref.abs().max()) > 1e-2, "a silent waveform would test nothing"
    decode.main(["--dumpdir", str(dump), "--outdir", str(tmp_path / "wav"), "--checkpoint",
                 str(tmp_path / "checkpoint-1steps.pkl"), "--batch-size", "2", "--verbose", "0"])
    model.remove_weight_norm()
    model = model.to(device).eval()
    model.pqmf = layers.PQMF(subbands=4).to(device)
    differ = total = 0
    for utt, mel in mels.items():
        pcm, rate = decode.read_wav_pcm16(str(tmp_path / "wav" / f"{utt}_gen.wav"))
        with torch.no_grad():
            want = to_pcm16(model.inference(torch.from_numpy(mel).to(device)).reshape(-1)).cpu().numpy()
        assert rate == 24000 and pcm.shape == want.shape == (mel.shape[0] * model.upsample_factor * 4,)
        delta = np.abs(pcm.astype(np.int32) - want.astype(np.int32))
        assert delta.max() <= 1, f"{utt}: {delta.max()} LSB"
        differ, total = differ + int((delta != 0).sum()), total + delta.size
    print(f"samples that differ by 1 LSB: {differ} of {total} ({100.0 * differ / total:.3f} %)")
    assert differ / total < 0.01
