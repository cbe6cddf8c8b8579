"""GPU: the slotted forms of the Parallel WaveGAN look-ahead stream's launches (csrc/wavenet_stream.hip,
csrc/wavenet_stream_bf16.hip, csrc/elementwise_slots.hip) and utils.PWGStreamPool on them -- a
slotted launch against the delayed launches of its items bit for bit, fresh and paused items, the seeded ``conv_in``, and a
pool of staggered utterances against one ``PWGLookaheadStream`` per utterance.  Every comparison is ``torch.equal``."""
import functools
import itertools

import pytest
import torch

from parallelwavegan_amd import models, ops
from parallelwavegan_amd.layers.causal_conv import SlotPosition, slot_table_rows_in
from parallelwavegan_amd.layers.residual_block import WaveNetResidualBlock
from parallelwavegan_amd.layers.upsample import ConvInUpsampleNetwork
from parallelwavegan_amd.utils import PWGLookaheadStream, PWGStreamPool
from parallelwavegan_amd.utils.streaming import slot_window
from tests.golden import synth
from tests.test_stream_pool_gpu import DELAY, _positions, _row
from tests.test_stream_pwg_lookahead_gpu import DEEP, SMALL
from tests.util import WAVE_TOL, max_abs, poison_lds, synth_for

pytestmark = pytest.mark.gpu

EXTRA = 37                     # the second c_delay of a dilation is d + EXTRA: an unaligned read of the conditioning line
LAYER_CHUNKS = (5, 64, 65, 130)  # the layer kernel's column tile is 64: below, at, above, more than two workgroups
SKIP_SCALE = 0.5


def _nan(device, *shape):
    return torch.full(shape, float("nan"), device=device)


def _kind(lo, hi, t_out):
    return "empty" if lo >= hi else "full" if (lo, hi) == (0, t_out) else "low" if lo else "high"


# ---- 1. / 2. the gated layer -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _block_state(d):
    torch.manual_seed(3000 + d)
    blk = WaveNetResidualBlock(dilation=d)
    for cv in blk.fused_convs():
        cv.apply_weight_norm()
    with torch.no_grad():
        for p in blk.parameters():
            p.add_(0.1 * torch.randn_like(p))
    return blk.state_dict()


def _block(d, device):
    blk = WaveNetResidualBlock(dilation=d)
    for cv in blk.fused_convs():
        cv.apply_weight_norm()
    blk.load_state_dict(_block_state(d))
    return blk.to(device).eval()


class _LayerCase:
    """One gated layer, one chunk size, ``batch`` items: inputs, state and the two launches."""

    def __init__(self, blk, precision, n, batch, c_delay, device, seed):
        gen = torch.Generator().manual_seed(seed)
        rand = lambda *shape: torch.randn(*shape, generator=gen).to(device)  # noqa: E731
        d = blk.conv.dilation
        self.blk, self.precision, self.n, self.batch, self.c_delay, self.d, self.device = blk, precision, n, batch, c_delay, d, device
        self.x, self.c, self.skips = rand(batch, 64, n), rand(batch, 80, n), rand(batch, 64, n)
        self.hist, self.sline, self.cline = rand(batch, 64, 2 * d), rand(batch, 64, d), rand(batch, 80, c_delay + 5)

    def _outs(self, batch):
        return _nan(self.device, batch, 64, 2 * self.d), _nan(self.device, batch, 64, self.d)

    def delayed(self, i, valid, fresh, skip=True):
        """Item ``i`` alone through the delayed launch -> (x_out, skips_out, hist_out, skip_line_out)."""
        cut = lambda t: t[i:i + 1].contiguous()  # noqa: E731
        h, s = self._outs(1)
        xo, so = self.blk.lookahead_forward(cut(self.x), cut(self.c), None if fresh else cut(self.cline), self.c_delay,
                                            (None if fresh else cut(self.hist), h), cut(self.skips) if skip else None,
                                            (None if fresh else cut(self.sline), s), valid, skip_scale=SKIP_SCALE,
                                            precision=self.precision)
        return xo, so, h, s

    def slotted(self, rows, skip=True, x=None, c=None, skips=None, hist=None, sline=None, cline=None):
        """All items through one slotted launch; the keyword tensors replace the case's."""
        pick = lambda given, own: own if given is None else given  # noqa: E731
        h, s = self._outs(self.batch)
        table = torch.tensor(rows, dtype=torch.int32, device=self.device)
        xo, so = self.blk.lookahead_forward(pick(x, self.x), pick(c, self.c), pick(cline, self.cline), self.c_delay,
                                            (pick(hist, self.hist), h), pick(skips, self.skips) if skip else None,
                                            (pick(sline, self.sline), s), SlotPosition(table, 1, DELAY, None),
                                            skip_scale=SKIP_SCALE, precision=self.precision)
        return xo, so, h, s


WHAT = ("x_out", "skips_out", "hist_out", "skip_line_out")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("d", [1, 4, 512])
def test_layer_uniform_table_equals_the_delayed_launch(d, precision, device):
    blk = _block(d, device)
    for c_delay, n in itertools.product((d, d + EXTRA), LAYER_CHUNKS):
        case = _LayerCase(blk, precision, n, 2, c_delay, device, 11 * d + n)
        seen = set()
        for name, (before, left) in _positions(1).items():
            lo, hi = valid = slot_window(DELAY, 1, n, before, left)
            seen.add(_kind(lo, hi, n))
            fresh = before == 0
            # a fresh item does not read its state: the buffers hold NaN there
            state = {k: _nan(device, *getattr(case, k).shape) for k in ("hist", "sline", "cline")} if fresh else {}
            for skip in (True, False):
                got = case.slotted([_row(before, left)] * 2, skip, **state)
                for i in range(2):
                    want = case.delayed(i, valid, fresh, skip)
                    for g, w, what in zip(got, want, WHAT[:4 if skip else 3]):
                        assert torch.equal(g[i:i + 1], w), (d, precision, c_delay, n, name, skip, i, what)
        assert seen == {"empty", "full", "low", "high"}, (n, seen)


def _mixed_items(rate):
    """The six items of a mixed table -> (positions, {paused item: is it fresh})."""
    pos = _positions(rate)
    return [pos["start"], pos["low edge"], pos["full"], (3, None), pos["high edge"], (0, None)], {3: False, 5: True}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("d", [4, 512])
def test_layer_mixed_table(d, precision, device):
    """Items at different positions in one launch, a paused and a fresh paused one among them; again under poisoned LDS."""
    blk = _block(d, device)
    for n in (5, 130):
        case = _LayerCase(blk, precision, n, 6, d + EXTRA, device, 13 * d + n)
        items, paused = _mixed_items(1)
        rows = [_row(b, left, i in paused) for i, (b, left) in enumerate(items)]
        # what a fresh item must not read, and what a paused one must not read, holds NaN
        moved = {k: getattr(case, k).clone() for k in ("x", "c", "skips", "hist", "sline", "cline")}
        for i in paused:
            for k in ("x", "c", "skips"):
                moved[k][i] = float("nan")
        for i in (0, 5):
            for k in ("hist", "sline", "cline"):
                moved[k][i] = float("nan")
        got = case.slotted(rows, True, **moved)
        with poison_lds():
            again = case.slotted(rows, True, **moved)
        for g, a, what in zip(got, again, WHAT):
            assert torch.equal(g, a), (d, precision, n, what)
        for i, (before, left) in enumerate(items):
            if i in paused:
                zeros = lambda t: torch.zeros_like(t[i])  # noqa: E731
                assert torch.equal(got[0][i], zeros(got[0])) and torch.equal(got[1][i], zeros(got[1])), (d, precision, n, i)
                for g, kept in zip(got[2:], (case.hist, case.sline)):
                    assert torch.equal(g[i], zeros(g) if paused[i] else kept[i]), (d, precision, n, i)
                continue
            want = case.delayed(i, slot_window(DELAY, 1, n, before, left), before == 0)
            for g, w, what in zip(got, want, WHAT):
                assert torch.equal(g[i:i + 1], w), (d, precision, n, i, what)


# ---- 3. the stretch stage and the delay line -------------------------------------------------------------------------
STAGE_CHUNKS = (1, 5, 33)
CH = 7  # channels per item (odd: an item's rows are no multiple of anything)


def _stage_case(scale, n, batch, device, seed):
    gen = torch.Generator().manual_seed(seed)
    rand = lambda *shape: torch.randn(*shape, generator=gen).to(device)  # noqa: E731
    return rand(batch, CH, n), rand(batch, CH, 2), rand(2 * scale + 1)


def _stage_delayed(x, hist, w, scale, act, i, valid, fresh):
    h = _nan(x.device, 1, CH, 2)
    y = ops.stretch_conv_stream_delayed(x[i:i + 1].contiguous(), None if fresh else hist[i:i + 1].contiguous(), h, w, scale,
                                        1, act, 0.2, valid)
    return y, h


def _stage_slotted(x, hist, w, scale, act, rows):
    h = _nan(x.device, x.shape[0], CH, 2)
    table = torch.tensor(rows, dtype=torch.int32, device=x.device)
    return ops.stretch_conv_stream_slots(x, hist, h, w, scale, 1, act, 0.2, slots=table, rate=scale, delay=DELAY), h


@pytest.mark.parametrize("act", [None, "leaky_relu"])
@pytest.mark.parametrize("scale", [4, 5])
def test_stage_equals_the_delayed_launch(scale, act, device):
    for n in STAGE_CHUNKS:
        t_out = n * scale
        # a uniform table at every position
        x, hist, w = _stage_case(scale, n, 2, device, 100 * scale + n)
        seen = set()
        for name, (before, left) in _positions(scale).items():
            lo, hi = valid = slot_window(DELAY, scale, t_out, before, left)
            seen.add(_kind(lo, hi, t_out))
            fresh = before == 0
            got = _stage_slotted(x, _nan(device, *hist.shape) if fresh else hist, w, scale, act, [_row(before, left)] * 2)
            for i in range(2):
                for g, want, what in zip(got, _stage_delayed(x, hist, w, scale, act, i, valid, fresh), ("y", "hist_out")):
                    assert torch.equal(g[i:i + 1], want), (scale, act, n, name, i, what)
        assert seen >= {"empty", "full"} and (n < 33 or seen == {"empty", "full", "low", "high"}), (n, seen)
        # a mixed table
        x, hist, w = _stage_case(scale, n, 6, device, 200 * scale + n)
        items, paused = _mixed_items(scale)
        rows = [_row(b, left, i in paused) for i, (b, left) in enumerate(items)]
        xm, hm = x.clone(), hist.clone()
        for i in paused:
            xm[i] = float("nan")
        for i in (0, 5):
            hm[i] = float("nan")
        y, h = _stage_slotted(xm, hm, w, scale, act, rows)
        for i, (before, left) in enumerate(items):
            if i in paused:
                assert torch.equal(y[i], torch.zeros_like(y[i])), (scale, act, n, i)
                assert torch.equal(h[i], torch.zeros_like(h[i]) if paused[i] else hist[i]), (scale, act, n, i)
                continue
            want = _stage_delayed(x, hist, w, scale, act, i, slot_window(DELAY, scale, t_out, before, left), before == 0)
            assert torch.equal(y[i:i + 1], want[0]) and torch.equal(h[i:i + 1], want[1]), (scale, act, n, i)


LINE = 5  # columns of the delay line: the chunks 1, 5, 33 are below, at and above it


@pytest.mark.parametrize("delayed", [False, True])
def test_delay_line_equals_the_lock_step_line(delayed, device):
    for n in STAGE_CHUNKS:
        gen = torch.Generator().manual_seed(300 + n)
        x, line = torch.randn(6, CH, n, generator=gen).to(device), torch.randn(6, CH, LINE, generator=gen).to(device)
        items, paused = _mixed_items(1)
        for uniform in (None, "start", "full"):
            pos = items if uniform is None else [_positions(1)[uniform]] * 6
            stop = paused if uniform is None else {}
            rows = [_row(b, left, i in stop) for i, (b, left) in enumerate(pos)]
            xm, lm = x.clone(), line.clone()
            for i, (before, _) in enumerate(pos):
                if i in stop:
                    xm[i] = float("nan")
                if before == 0:
                    lm[i] = float("nan")
            out = _nan(device, 6, CH, LINE)
            y = ops.delay_line_slots_forward(xm, lm, out, torch.tensor(rows, dtype=torch.int32, device=device), delayed)
            assert (y is not None) == delayed
            for i, (before, _) in enumerate(pos):
                if i in stop:
                    assert torch.equal(out[i], torch.zeros_like(out[i]) if stop[i] else line[i]), (n, uniform, i)
                    assert not delayed or torch.equal(y[i], torch.zeros_like(y[i])), (n, uniform, i)
                    continue
                want_out = _nan(device, 1, CH, LINE)
                want = ops.delay_line_forward(x[i:i + 1].contiguous(), None if before == 0 else line[i:i + 1].contiguous(),
                                              want_out, delayed)
                assert torch.equal(out[i:i + 1], want_out), (n, uniform, i)
                assert not delayed or torch.equal(y[i:i + 1], want), (n, uniform, i)


# ---- 4. the seed and conv_in over the second table -------------------------------------------------------------------
def test_seed_and_conv_in_over_the_second_table(device):
    torch.manual_seed(5)
    w, n = 2, 4
    net = ConvInUpsampleNetwork([4, 4], aux_context_window=w).to(device).eval()
    cv = net.conv_in
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(5, 80, n, generator=gen).to(device)
    old = torch.randn(5, 80, 2 * w, generator=gen).to(device)
    # fresh running, three frames in, fresh paused, paused, fresh running
    first = [_row(0, None), _row(3, None), _row(0, None, True), _row(2, None, True), _row(0, 2)]
    table = torch.tensor(first, dtype=torch.int32, device=device)
    hist = old.clone()
    assert ops.slot_seed_history(x, hist, table) is hist
    for i in (0, 4):  # every column of a fresh running item is column 0 of its x
        assert torch.equal(hist[i], x[i, :, :1].expand(-1, 2 * w)), i
    for i in (1, 2, 3):  # nobody else changes
        assert torch.equal(hist[i], old[i]), i
    # conv_in with delay + rate over the second table against the seeded delayed launch of each item
    second = torch.tensor(slot_table_rows_in(first), dtype=torch.int32, device=device)
    assert second[:, 0].min().item() >= 1  # no item of it is fresh
    h_out = _nan(device, 5, 80, 2 * w)
    y = ops.conv1d_stream_slots_forward(net._lookahead_desc(5, n), x, hist, h_out, cv.packed_weight(), None, slots=second,
                                        rate=1, delay=w + 1)
    for i, (before, left, fresh) in ((0, (0, None, True)), (1, (3, None, False)), (4, (0, 2, True))):
        want_h = _nan(device, 1, 80, 2 * w)
        xi = x[i:i + 1].contiguous()
        seeded = xi[:, :, :1].expand(-1, -1, 2 * w).contiguous() if fresh else old[i:i + 1].contiguous()
        valid = slot_window(w, 1, n, before, left)
        assert valid == slot_window(w + 1, 1, n, before + 1, None if left is None else left - 1)
        want = ops.conv1d_stream_delayed_forward(net._lookahead_desc(1, n), xi, seeded, want_h, cv.packed_weight(), None,
                                                 valid=valid)
        assert torch.equal(y[i:i + 1], want) and torch.equal(h_out[i:i + 1], want_h), i
    for i in (2, 3):  # paused in the second table: zeros out, history through
        assert torch.equal(y[i], torch.zeros_like(y[i])) and torch.equal(h_out[i], old[i]), i


# ---- 5. refusals -----------------------------------------------------------------------------------------------------
def test_slotted_entries_want_every_state_buffer_and_the_table(device):
    blk = _block(4, device)
    z = lambda *shape: torch.zeros(*shape, device=device)  # noqa: E731
    table = torch.zeros(1, ops.SLOT_INTS, dtype=torch.int32, device=device)
    x, c, cline = z(1, 64, 8), z(1, 80, 8), z(1, 80, 9)
    hist, sline = [z(1, 64, 8), z(1, 64, 8)], [z(1, 64, 4), z(1, 64, 4)]

    def layer(precision, position, hist_in=hist[0], c_line=cline, line_in=sline[0]):
        return blk.lookahead_forward(x, c, c_line, 4, (hist_in, hist[1]), z(1, 64, 8), (line_in, sline[1]), position,
                                     precision=precision)

    for precision in ("fp32", "bf16"):
        where = SlotPosition(table, 1, 0, None)
        with pytest.raises(RuntimeError, match="hist_in"):
            layer(precision, where, hist_in=None)
        with pytest.raises(RuntimeError, match="c_line"):
            layer(precision, where, c_line=None)
        with pytest.raises(RuntimeError, match="skip_line_in"):
            layer(precision, where, line_in=None)
        with pytest.raises(RuntimeError, match="slots"):
            layer(precision, SlotPosition(None, 1, 0, None))
    s, w = z(1, CH, 4), z(9)
    h2 = [z(1, CH, 2), z(1, CH, 2)]
    with pytest.raises(RuntimeError, match="hist_in"):
        ops.stretch_conv_stream_slots(s, None, h2[1], w, 4, slots=table)
    with pytest.raises(RuntimeError, match="slots"):
        ops.stretch_conv_stream_slots(s, h2[0], h2[1], w, 4)
    with pytest.raises(RuntimeError, match="line_in"):
        ops.delay_line_slots_forward(s, None, z(1, CH, 3), table)
    with pytest.raises(RuntimeError, match="slots"):
        ops.delay_line_slots_forward(s, z(1, CH, 3), z(1, CH, 3), None)
    with pytest.raises(RuntimeError, match="hist"):
        ops.slot_seed_history(s, None, table)
    with pytest.raises(RuntimeError, match="slots"):
        ops.slot_seed_history(s, z(1, CH, 3), None)


# ---- 6. the pool -----------------------------------------------------------------------------------------------------
LENGTHS = (1, 3, 9, 14, 23)  # some shorter than the latency of 4.1 frames, none a multiple of the chunk
UP, LATENCY = 16, 66


@functools.lru_cache(maxsize=None)
def _utterances(lengths=LENGTHS):
    """[((T, 80) features, (T * up,) noise) on the CPU]: computed once, never modified."""
    return [(synth.synth_input(f"pwgpool{i}", (t, 80), seed=70 + i), synth.synth_input(f"pwgz{i}", (t * UP,), seed=80 + i))
            for i, t in enumerate(lengths)]


@functools.lru_cache(maxsize=None)
def _state(name):
    return synth_for(models.ParallelWaveGANGenerator(**{"small": SMALL, "deep": DEEP}[name]), 41, 1.0)


def _model(name, device):
    m = models.ParallelWaveGANGenerator(**{"small": SMALL, "deep": DEEP}[name])
    m.load_state_dict(_state(name))
    return m.to(device).eval()


def _single(stream, f, z, cut=2):
    """One utterance through a batch-1 look-ahead stream, pushes and flush together."""
    stream.reset()
    parts = [stream.push(f[:cut], z[:cut * stream.up]), stream.push(f[cut:], z[cut * stream.up:]), stream.flush()]
    return torch.cat(parts, -1)[0]


_REFERENCE = {}


def _reference(model, precision):
    if precision not in _REFERENCE:
        s = PWGLookaheadStream(model, batch=1, use_graph=False, precision=precision)
        _REFERENCE[precision] = [_single(s, f, z) for f, z in _utterances()]
    return _REFERENCE[precision]


def _drive(pool, utterances):
    """All utterances through the pool: staggered ``open()``, the irregular ``feed()`` sizes of the HiFi-GAN pool test ->
    (per utterance the concatenated emissions, facts about the run)."""
    pending, active, used = list(range(len(utterances))), {}, []
    outs = {i: [] for i in pending}
    sizes = itertools.cycle((1, 3, 0, 6, 2))
    facts = dict(pauses=0, reused=0, steps=0)
    for tick in range(400):
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
            f, z = utterances[st[0]]
            n = min(next(sizes), f.shape[0] - st[1])
            pool.feed(slot, f[st[1]:st[1] + n], z[st[1] * pool.up:(st[1] + n) * pool.up])
            st[1] += n
            if st[1] == f.shape[0]:
                pool.end(slot)
                st[2] = True
        out = pool.step()
        facts["steps"] += bool(out)
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
    return [torch.cat(outs[i], -1) for i in range(len(utterances))], facts


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_pool_equals_one_lookahead_stream_per_utterance(precision, device):
    model = _model("small", device)
    refs = _reference(model, precision)
    pool = PWGStreamPool(model, slots=3, chunk_frames=4, use_graph=False, precision=precision)
    assert (pool.latency_samples, pool.up, pool.precision) == (LATENCY, UP, precision)
    assert pool.state_bytes == 2 * 4 * sum(t.numel() for t in pool._halves[0]) > 0
    got, facts = _drive(pool, _utterances())
    print("pwg pool", precision, facts)
    assert facts["pauses"] > 0 and facts["reused"] > 0
    for i, (y, ref) in enumerate(zip(got, refs)):
        assert y.shape == (LENGTHS[i] * UP,) and torch.equal(y, ref), (precision, i)
    if precision == "fp32":
        for i, (f, z) in enumerate(_utterances()):
            with torch.no_grad():
                full = model.inference(f.to(device), x=z.reshape(-1, 1).to(device)).reshape(-1)
            assert max_abs(got[i], full) <= WAVE_TOL, i
    # graph mode: one pair of graphs from the first step on, the same bits
    graphed = PWGStreamPool(model, slots=3, chunk_frames=4, use_graph=True, precision=precision)
    assert graphed.graphs_captured == 0
    again, facts = _drive(graphed, _utterances())
    assert graphed.graphs_captured == 2 and facts["steps"] > 10
    for i, (y, ref) in enumerate(zip(again, refs)):
        assert torch.equal(y, ref), (precision, i)
    # a second round in the same pool: every slot is reused
    assert all(torch.equal(y, ref) for y, ref in zip(_drive(graphed, _utterances())[0], refs))
    assert graphed.graphs_captured == 2


# ---- 7. deep dilations, reuse without clearing -----------------------------------------------------------------------
def test_deep_pool_and_slot_reuse_without_clearing(device):
    model = _model("deep", device)
    assert PWGLookaheadStream.latency_samples_of(model) == 1075
    utts = _utterances((5, 70))
    s = PWGLookaheadStream(model, batch=1, use_graph=False)
    refs = [_single(s, f, z) for f, z in utts]

    def run(pool, which):
        slots = {}
        for i in which:
            slots[pool.open()] = i
            pool.feed(list(slots)[-1], *utts[i])
            pool.end(list(slots)[-1])
        outs = {i: [] for i in which}
        while pool.open_slots:
            for slot, y in pool.step().items():
                outs[slots[slot]].append(y)
        return {i: torch.cat(ys) for i, ys in outs.items()}

    pool = PWGStreamPool(model, slots=2, chunk_frames=8, use_graph=False)
    got = run(pool, (0, 1))
    for i in (0, 1):
        assert got[i].shape == (utts[i][0].shape[0] * UP,) and torch.equal(got[i], refs[i]), i
    # the slots now hold the state of d = 512 utterances; the short utterance in either gives the bits of a fresh pool
    again = run(pool, (0,))[0]
    assert torch.equal(again, refs[0])
    assert torch.equal(run(pool, (1, 0))[0], refs[0])


# ---- 8. normalisation ------------------------------------------------------------------------------------------------
def test_pool_normalizes_like_the_stream(device):
    model = _model("small", device)
    gen = torch.Generator().manual_seed(17)
    mean, scale = torch.randn(80, generator=gen) * 0.1, 1.0 + 0.1 * torch.rand(80, generator=gen)
    model.register_buffer("mean", mean.to(device))
    model.register_buffer("scale", scale.to(device))
    f, z = torch.randn(9, 80, generator=gen) * scale + mean, torch.randn(9 * UP, generator=gen)
    s = PWGLookaheadStream(model, normalize_before=True, use_graph=False)
    ref = torch.cat([s.push(f, z), s.flush()], -1)[0]
    for graph in (False, True):
        pool = PWGStreamPool(model, slots=2, chunk_frames=4, normalize_before=True, use_graph=graph)
        slot = pool.open()
        pool.feed(slot, f, z)
        pool.end(slot)
        outs = []
        while pool.open_slots:
            outs.append(pool.step()[slot])
        assert torch.equal(torch.cat(outs), ref), graph


# ---- 9. noise not given ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True])
def test_pool_draws_noise_outside_the_graph(use_graph, device):
    model = _model("small", device)
    f, z = _utterances()[3]  # 14 frames
    pool = PWGStreamPool(model, slots=2, chunk_frames=4, use_graph=use_graph)

    def run(noise_of):
        slot = pool.open()
        for at in range(0, 14, 7):
            pool.feed(slot, f[at:at + 7], noise_of(at))
        pool.end(slot)
        outs = []
        while pool.open_slots:
            outs.append(pool.step()[slot])
        kept = [y.clone() for y in outs]
        return outs, kept

    torch.manual_seed(3)
    drawn, kept = run(lambda at: None)
    other, _ = run(lambda at: None)
    zeros, _ = run(lambda at: torch.zeros(7 * UP))
    assert sum(y.shape[0] for y in drawn) == 14 * UP and all(torch.isfinite(y).all() for y in drawn)
    for y, k in zip(drawn, kept):  # the caller's tensors are not the graph's static buffer: later steps left them alone
        assert torch.equal(y, k)
    assert not torch.equal(torch.cat(drawn), torch.cat(other))   # two runs differ: a replay draws anew
    assert not torch.equal(torch.cat(drawn), torch.cat(zeros))
    # half given, half drawn: the first half is the single stream's (its samples depend on nothing later than its frames
    # plus the look-ahead, so compare what the first 7 frames alone determine: 7 * up - latency samples)
    mixed, _ = run(lambda at: z[:7 * UP] if at == 0 else None)
    s = PWGLookaheadStream(model, batch=1, use_graph=False)
    ref = s.push(f[:7], z[:7 * UP])[0]
    assert ref.shape[0] == 7 * UP - LATENCY and torch.equal(torch.cat(mixed)[:ref.shape[0]], ref)


# ---- 10. launch census -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_a_step_launches_only_slotted_kernels(precision, device):
    model = _model("small", device)
    pool = PWGStreamPool(model, slots=3, chunk_frames=4, use_graph=False, precision=precision)
    a, b = pool.open(), pool.open()
    f, z = _utterances()[2]
    pool.feed(a, f, z)
    pool.feed(b, *[t[:2 * k] for t, k in zip(_utterances()[1], (1, UP))])  # paused
    pool.step()                                                             # (packs the weight images)
    with ops.profile() as prof:
        out = pool.step()
    assert list(out) == [a]
    launches = {k: v["launches"] for k, v in prof.results.items() if "stream" in k or "line" in k or "seed" in k}
    layer = "wavenet_stream_bf16_slots_kernel" if precision == "bf16" else "wavenet_stream_slots_kernel"
    conv = "conv1d_stream_bf16_slots_kernel" if precision == "bf16" else "conv1d_stream_slots_kernel"
    assert launches == {layer: len(model.conv_layers), "stretch_conv_stream_slots_kernel": 2, "delay_line_slots_kernel": 2,
                        conv: 4, "slot_seed_history_kernel": 1}, launches  # conv: conv_in, first_conv, two last ones
    # nothing to run: nothing is launched
    pool.end(a)
    while a in pool.open_slots:
        pool.step()
    with ops.profile() as prof:
        assert pool.step() == {}
    assert not prof.results
