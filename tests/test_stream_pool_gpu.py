"""GPU: the slotted form of the streaming convolution (csrc/conv1d_stream.hip, csrc/conv1d_stream_bf16.hip) and
utils.StreamPool on it -- a slotted launch against the delayed launches of its items bit for bit,
fresh and paused items, and a pool of staggered utterances against one ``LookaheadStream`` per utterance."""
import functools
import itertools

import pytest
import torch

from parallelwavegan_amd import layers, models, ops
from parallelwavegan_amd.layers.causal_conv import lookahead_desc, lookahead_history_columns
from parallelwavegan_amd.utils import LookaheadStream, StreamPool
from parallelwavegan_amd.utils.streaming import slot_window
from tests.golden import synth
from tests.util import WAVE_TOL, max_abs, poison_lds, synth_for

pytestmark = pytest.mark.gpu

CHUNKS = (5, 16, 17, 33, 70)  # every column tile of the stream kernel (16 / 32 / 64 columns) and its edges
FUSED = dict(pre_act="leaky_relu", pre_slope=0.1, out_div=3.0)
D1, D2, DELAY = 7, 30, 22    # the addends' delay lines; the launch's output delay
FAR = 10 ** 6                # a position past every delay


def _layer(kind, device):
    torch.manual_seed(9)
    cv = layers.Conv1d(24, 40, 5, dilation=3, padding=6) if kind == "conv" else layers.ConvTranspose1d(24, 12, 8, 4, padding=2)
    return cv.to(device), (4 if kind == "up" else 1)


def _nan(device, *shape):
    return torch.full(shape, float("nan"), device=device)


def _positions(rate):
    """name -> (frames before, frames left or None): the start, a window cut at either end, full, and empty."""
    return {"start": (0, None), "low edge": ((DELAY - 1) // rate, None), "high edge": (FAR, -((DELAY - 1) // rate)),
            "full": (FAR, None), "full, end known": (FAR, 70), "empty": (FAR, -FAR)}


def _row(before, left, paused=False):
    sat = 0 if left is None else max(-2 ** 31 + 1, min(left, 2 ** 31 - 1))
    return [min(before, 2 ** 31 - 1), sat, (ops.SLOT_PAUSED if paused else 0) | (0 if left is None else ops.SLOT_LEFT_KNOWN), 0]


class _Case:
    """One layer, one chunk size, ``batch`` items: inputs, state and the two launches (everything on the device)."""

    def __init__(self, kind, precision, n, batch, device, seed):
        self.cv, self.s = _layer(kind, device)
        cv, s = self.cv, self.s
        gen = torch.Generator().manual_seed(seed)
        rand = lambda *shape: torch.randn(*shape, generator=gen).to(device)  # noqa: E731
        self.n, self.batch, self.device, self.bf16 = n, batch, device, precision == "bf16"
        self.h_cols, self.c_out, self.t_out = lookahead_history_columns(cv), cv.out_channels, n * s
        self.x, self.hist = rand(batch, 24, n), rand(batch, 24, self.h_cols)
        self.a1, self.a2 = rand(batch, self.c_out, self.t_out), rand(batch, self.c_out, self.t_out)
        self.l1, self.l2 = rand(batch, self.c_out, D1), rand(batch, self.c_out, D2)
        self.w = cv.packed_weight_bf16() if self.bf16 else cv.packed_weight()
        self.bias = cv.bias.detach()

    def _outs(self, batch):
        dev = self.device
        return (_nan(dev, batch, self.c_out, self.t_out), _nan(dev, batch, 24, self.h_cols), _nan(dev, batch, self.c_out, D1),
                _nan(dev, batch, self.c_out, D2))

    def delayed(self, i, valid, fresh):
        """Item ``i`` alone through the delayed launch -> (y, hist_out, line1_out, line2_out)."""
        cut = lambda t: t[i:i + 1].contiguous()  # noqa: E731
        y, h, o1, o2 = self._outs(1)
        fn = ops.conv1d_stream_delayed_forward_bf16 if self.bf16 else ops.conv1d_stream_delayed_forward
        fn(lookahead_desc(self.cv, 1, self.n, **FUSED), cut(self.x), None if fresh else cut(self.hist), h, self.w, self.bias,
           cut(self.a1), (None if fresh else cut(self.l1), o1), D1, cut(self.a2), (None if fresh else cut(self.l2), o2), D2,
           valid=valid, out=y)
        return y, h, o1, o2

    def slotted(self, rows, x=None, hist=None, a1=None, l1=None, a2=None, l2=None):
        """All items through one slotted launch; the keyword tensors replace the case's."""
        y, h, o1, o2 = self._outs(self.batch)
        table = torch.tensor(rows, dtype=torch.int32, device=self.device)
        fn = ops.conv1d_stream_slots_forward_bf16 if self.bf16 else ops.conv1d_stream_slots_forward
        pick = lambda given, own: own if given is None else given  # noqa: E731
        fn(lookahead_desc(self.cv, self.batch, self.n, **FUSED), pick(x, self.x), pick(hist, self.hist), h, self.w, self.bias,
           pick(a1, self.a1), (pick(l1, self.l1), o1), D1, pick(a2, self.a2), (pick(l2, self.l2), o2), D2, slots=table,
           rate=self.s, delay=DELAY, out=y)
        return y, h, o1, o2


# ---- 1. the slotted launch against the delayed one -----------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["conv", "up"])
def test_uniform_table_equals_the_delayed_launch(kind, precision, device):
    for n in CHUNKS:
        case = _Case(kind, precision, n, 2, device, 41 + n)
        seen = set()
        for name, (before, left) in _positions(case.s).items():
            lo, hi = valid = slot_window(DELAY, case.s, case.t_out, before, left)
            seen.add("empty" if lo >= hi else "full" if (lo, hi) == (0, case.t_out) else "low" if lo else "high")
            fresh = before == 0
            # a fresh item does not read its state: the buffers hold NaN there
            state = {k: _nan(device, *getattr(case, k).shape) for k in ("hist", "l1", "l2")} if fresh else {}
            got = case.slotted([_row(before, left)] * 2, **state)
            for i in range(2):
                want = case.delayed(i, valid, fresh)
                for g, w, what in zip(got, want, ("y", "hist_out", "line1", "line2")):
                    assert torch.equal(g[i:i + 1], w), (kind, precision, n, name, i, what)
        assert seen == {"empty", "full", "low", "high"}, (n, seen)


@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["conv", "up"])
def test_mixed_table(kind, precision, poison, device):
    """Items at different positions in one launch, a paused and a fresh paused one among them."""
    for n in (5, 33, 70):
        case = _Case(kind, precision, n, 6, device, 57 + n)
        pos = _positions(case.s)
        items = [pos["start"], pos["low edge"], pos["full"], (3, None), pos["high edge"], (0, None)]
        paused = {3: False, 5: True}  # item -> is it fresh
        rows = [_row(b, left, i in paused) for i, (b, left) in enumerate(items)]
        # what a fresh item must not read, and what a paused one must not read, holds NaN
        x, a1, a2 = case.x.clone(), case.a1.clone(), case.a2.clone()
        hist, l1, l2 = case.hist.clone(), case.l1.clone(), case.l2.clone()
        for i in paused:
            x[i], a1[i], a2[i] = float("nan"), float("nan"), float("nan")
        for i in (0, 5):
            hist[i], l1[i], l2[i] = float("nan"), float("nan"), float("nan")
        got = case.slotted(rows, x, hist, a1, l1, a2, l2)
        if poison:
            with poison_lds():
                again = case.slotted(rows, x, hist, a1, l1, a2, l2)
            for g, a in zip(got, again):
                assert torch.equal(g, a), (kind, precision, n)
            continue
        for i, (before, left) in enumerate(items):
            if i in paused:
                zeros = lambda t: torch.zeros_like(t[i])  # noqa: E731
                assert torch.equal(got[0][i], zeros(got[0])), (kind, precision, n, i)
                for g, kept in zip(got[1:], (case.hist, case.l1, case.l2)):
                    assert torch.equal(g[i], zeros(g) if paused[i] else kept[i]), (kind, precision, n, i)
                continue
            want = case.delayed(i, slot_window(DELAY, case.s, case.t_out, before, left), before == 0)
            for g, w, what in zip(got, want, ("y", "hist_out", "line1", "line2")):
                assert torch.equal(g[i:i + 1], w), (kind, precision, n, i, what)


def test_slotted_launch_wants_every_state_buffer(device):
    cv, _ = _layer("conv", device)
    desc = lookahead_desc(cv, 1, 4)
    x, add = torch.zeros(1, 24, 4, device=device), torch.zeros(1, 40, 4, device=device)
    hist, line = [torch.zeros(1, 24, 12, device=device) for _ in range(2)], [torch.zeros(1, 40, 7, device=device) for _ in range(2)]
    table = torch.zeros(1, ops.SLOT_INTS, dtype=torch.int32, device=device)
    with pytest.raises(RuntimeError, match="hist_in"):
        ops.conv1d_stream_slots_forward(desc, x, None, hist[1], cv.packed_weight(), slots=table)
    with pytest.raises(RuntimeError, match="add_hist_in"):
        ops.conv1d_stream_slots_forward(desc, x, hist[0], hist[1], cv.packed_weight(), None, add, (None, line[1]), 7, slots=table)
    with pytest.raises(RuntimeError, match="slots"):
        ops.conv1d_stream_slots_forward(desc, x, hist[0], hist[1], cv.packed_weight())


# ---- 2. the pool ---------------------------------------------------------------------------------------------------
LENGTHS = (1, 3, 9, 14, 23)  # some shorter than the latency of 7.6 frames, none a multiple of the chunk
UP, LATENCY = 24, 182


@functools.lru_cache(maxsize=None)
def _utterances():
    """(state dict, [(T, 80) features on the CPU]): computed once, never modified."""
    sd = synth_for(models.HiFiGANGenerator(**synth.HIFIGAN_TINY), 21, 1.0)
    return sd, [synth.synth_input(f"pool{i}", (t, 80), seed=60 + i) for i, t in enumerate(LENGTHS)]


def _model(device):
    m = models.HiFiGANGenerator(**synth.HIFIGAN_TINY)
    m.load_state_dict(_utterances()[0])
    return m.to(device).eval()


_REFERENCE = {}


def _reference(model, precision):
    """Per utterance what ``LookaheadStream(batch=1)`` emits for it, pushes and flush together; once per precision."""
    if precision not in _REFERENCE:
        s, refs = LookaheadStream(model, batch=1, use_graph=False, precision=precision), []
        for f in _utterances()[1]:
            s.reset()
            refs.append(torch.cat([s.push(f[:2]), s.push(f[2:]), s.flush()], -1)[0])
        _REFERENCE[precision] = refs
    return _REFERENCE[precision]


def _drive(pool):
    """All utterances through the pool: staggered ``open()``, irregular ``feed()`` sizes -> (per utterance the
    concatenated emissions, facts about the run)."""
    feats = _utterances()[1]
    pending, active, used = list(range(len(feats))), {}, []
    outs = {i: [] for i in pending}
    sizes = itertools.cycle((1, 3, 0, 6, 2))
    facts = dict(pauses=0, reused=0, empty_steps=0, steps=0)
    for tick in range(200):
        if not pending and not active:
            break
        if pending and tick % 2 == 0 and len(pool.open_slots) < pool.slots:
            slot = pool.open()
            facts["reused"] += slot in used
            used.append(slot)
            active[slot] = [pending.pop(0), 0, False]
        for slot, st in active.items():
            if st[2]:
                continue
            n = min(next(sizes), feats[st[0]].shape[0] - st[1])
            pool.feed(slot, feats[st[0]][st[1]:st[1] + n])
            st[1] += n
            if st[1] == feats[st[0]].shape[0]:
                pool.end(slot)
                st[2] = True
        out = pool.step()
        facts["steps"] += bool(out)
        facts["empty_steps"] += not out
        for slot, st in list(active.items()):
            if slot in out:
                outs[st[0]].append(out[slot])
            elif out:
                facts["pauses"] += 1
                assert not st[2]  # (an ended slot runs in every step)
            if slot not in pool.open_slots:
                assert st[2]
                del active[slot]
    assert not pending and not active and pool.open_slots == []
    assert pool.step() == {}
    return [torch.cat(outs[i], -1) for i in range(len(feats))], facts


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_pool_equals_one_lookahead_stream_per_utterance(precision, device):
    model = _model(device)
    refs = _reference(model, precision)
    pool = StreamPool(model, slots=3, chunk_frames=4, use_graph=False, precision=precision)
    assert (pool.latency_samples, pool.up, pool.precision) == (LATENCY, UP, precision)
    assert pool.state_bytes == 2 * 4 * sum(t.numel() for t in pool._halves[0]) > 0
    got, facts = _drive(pool)
    print("pool", precision, facts)
    assert facts["pauses"] > 0 and facts["reused"] > 0
    for i, (y, ref) in enumerate(zip(got, refs)):
        assert y.shape == (LENGTHS[i] * UP,) and torch.equal(y, ref), (precision, i)
    if precision == "fp32":
        for i, f in enumerate(_utterances()[1]):
            with torch.no_grad():
                full = model(f.t().unsqueeze(0).contiguous().to(device))[0, 0]
            assert max_abs(got[i], full) <= WAVE_TOL, i
    # graph mode: one pair of graphs from the first step on, the same bits
    graphed = StreamPool(model, slots=3, chunk_frames=4, use_graph=True, precision=precision)
    assert graphed.graphs_captured == 0
    again, facts = _drive(graphed)
    assert graphed.graphs_captured == 2 and facts["steps"] > 10
    for i, (y, ref) in enumerate(zip(again, refs)):
        assert torch.equal(y, ref), (precision, i)
    # a second round in the same pool: every slot is reused
    assert all(torch.equal(y, ref) for y, ref in zip(_drive(graphed)[0], refs)) and graphed.graphs_captured == 2


def test_pool_normalizes_and_pads_after_normalisation(device):
    model = _model(device)
    gen = torch.Generator().manual_seed(17)
    mean, scale = torch.randn(80, generator=gen) * 0.1, 1.0 + 0.1 * torch.rand(80, generator=gen)
    model.register_buffer("mean", mean.to(device))
    model.register_buffer("scale", scale.to(device))
    f = torch.randn(9, 80, generator=gen) * scale + mean
    s = LookaheadStream(model, normalize_before=True, use_graph=False)
    ref = torch.cat([s.push(f), s.flush()], -1)[0]
    for graph in (False, True):
        pool = StreamPool(model, slots=2, chunk_frames=4, normalize_before=True, use_graph=graph)
        slot = pool.open()
        pool.feed(slot, f)
        pool.end(slot)
        outs = []
        while pool.open_slots:
            outs.append(pool.step()[slot])
        assert torch.equal(torch.cat(outs), ref), graph


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_a_step_is_one_slotted_launch_per_layer(precision, device):
    model = _model(device)
    pool = StreamPool(model, slots=3, chunk_frames=4, use_graph=False, precision=precision)
    a, b = pool.open(), pool.open()
    pool.feed(a, _utterances()[1][2])
    pool.feed(b, _utterances()[1][1][:2])  # paused
    pool.step()                            # (packs the weight images)
    with ops.profile() as prof:
        out = pool.step()
    assert list(out) == [a]
    stream_kernels = {k: v["launches"] for k, v in prof.results.items() if "stream" in k}
    slotted = "conv1d_stream_bf16_slots_kernel" if precision == "bf16" else "conv1d_stream_slots_kernel"
    assert stream_kernels == {slotted: len(model.lookahead_plan())}, stream_kernels
    # nothing to run: nothing is launched
    pool.end(a)
    while a in pool.open_slots:
        pool.step()
    with ops.profile() as prof:
        assert pool.step() == {}
    assert not prof.results
