"""GPU: the slotted-mirrored form of the streaming convolution (csrc/conv1d_stream.hip), the slotted PQMF synthesis
(csrc/pqmf.hip) and utils.MelGANStreamPool on them -- a slotted-mirrored launch against the mirrored
launches of its items bit for bit, fresh and paused items, the slotted synthesis against the stream synthesis of its
items, and a pool of staggered (multi-band) MelGAN utterances against one ``MelGANLookaheadStream`` per utterance."""
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

from parallelwavegan_amd import layers, models, ops
from parallelwavegan_amd.layers.causal_conv import launch_is_mirrored, mirrored_desc
from parallelwavegan_amd.utils import MelGANLookaheadStream, MelGANStreamPool
from parallelwavegan_amd.utils.streaming import slot_mirror_window, slot_window
from tests.golden import synth
from tests.util import WAVE_TOL, load_golden, max_abs, poison_lds, synth_for

pytestmark = pytest.mark.gpu

CHUNKS = (5, 16, 17, 33, 70)  # every column tile of the stream kernel (16 / 32 / 64 columns) and its edges
LAYERS = [(7, 1), (3, 9), (3, 27)]  # (kernel, dilation): paddings 3, 9, 27
RATE, IN_DELAY = 2, 40  # columns per frame; the INPUT's delay, so in_lo = 40 - 2 * before and in_hi = 40 + 2 * left
FAR = 10 ** 6           # a position past every delay
SLOPE = 0.2
FORWARD_TOL = 2e-5      # tests/test_stream_melgan_lookahead_gpu.py: a look-ahead stream against `forward`


def _nan(device, *shape):
    return torch.full(shape, float("nan"), device=device)


def _row(before, left, paused=False):
    return [before, 0 if left is None else left,
            (ops.SLOT_PAUSED if paused else 0) | (0 if left is None else ops.SLOT_LEFT_KNOWN), 0]


def _positions(p):
    """name -> (frames before, frames left or None).  Left edge ``40 - 2 * before``, right edge ``40 + 2 * left``."""
    return {
        "fresh": (0, None),                                # left edge at 40: in the chunk only for n = 70
        "left edge in the chunk": (19, None),              # 2
        "left edge in the history": (21, None),            # -2
        "left edge at a 16-column boundary": (12, None),   # 16
        "left edge saturated": (FAR, None),
        "right edge in the chunk": (FAR, -18),             # 4
        "right edge in the history": (FAR, -21),           # -2
        "right edge at a 16-column boundary": (FAR, -12),  # 16
        "right edge saturated, empty": (FAR, -FAR),
        "right edge saturated, full": (FAR, FAR),
        "both edges in one window": (19, (2 + p + 1 - IN_DELAY) // 2),  # [2, 2 + p + 1): the shortest utterance
    }


class _Layer:
    """One reflect-padded layer, one chunk size, ``batch`` items: inputs, state and the two launches."""

    def __init__(self, k, d, n, batch, device, seed):
        torch.manual_seed(9)
        self.p = (k - 1) * d // 2
        self.cv = layers.Conv1d(24, 40, k, dilation=d, padding=self.p, pad_mode="reflect").to(device)
        self.fused = dict(pre_act="leaky_relu", pre_slope=SLOPE, **({"post_act": "tanh"} if k == 7 else {}))
        gen = torch.Generator().manual_seed(seed)
        self.n, self.batch, self.device, self.delay = n, batch, device, IN_DELAY + self.p
        self.x = torch.randn(batch, 24, n, generator=gen).to(device)
        self.hist = torch.randn(batch, 24, 2 * self.p, generator=gen).to(device)
        self.w, self.bias = self.cv.packed_weight(), self.cv.bias.detach()

    def _outs(self, batch):
        return _nan(self.device, batch, 40, self.n), _nan(self.device, batch, 24, 2 * self.p)

    def mirrored(self, i, before, left):
        """Item ``i`` alone through the mirrored launch with the windows the table row stands for -> (y, hist_out)."""
        y, h = self._outs(1)
        ops.conv1d_stream_mirrored_forward(
            mirrored_desc(self.cv, 1, self.n, **self.fused), self.x[i:i + 1].contiguous(),
            None if before == 0 else self.hist[i:i + 1].contiguous(), h, self.w, self.bias,
            slot_mirror_window(self.delay, self.p, RATE, self.n, before, left),
            slot_window(self.delay, RATE, self.n, before, left), out=y)
        return y, h

    def slotted(self, rows, x=None, hist=None):
        y, h = self._outs(self.batch)
        table = torch.tensor(rows, dtype=torch.int32, device=self.device)
        ops.conv1d_stream_slots_mirrored_forward(
            mirrored_desc(self.cv, self.batch, self.n, **self.fused), self.x if x is None else x,
            self.hist if hist is None else hist, h, self.w, self.bias, slots=table, rate=RATE, delay=self.delay, out=y)
        return y, h


# ---- 1. the slotted-mirrored launch against the mirrored one ---------------------------------------------------------
@pytest.mark.parametrize("k,d", LAYERS)
def test_uniform_table_equals_the_mirrored_launch(k, d, device):
    for n in CHUNKS:
        case = _Layer(k, d, n, 2, device, 41 + n)
        nonzero = 0
        for name, (before, left) in _positions(case.p).items():
            # a fresh item does not read its history: the buffer holds NaN there
            got = case.slotted([_row(before, left)] * 2, hist=_nan(device, *case.hist.shape) if before == 0 else None)
            for i in range(2):
                want = case.mirrored(i, before, left)
                for g, w, what in zip(got, want, ("y", "hist_out")):
                    assert torch.equal(g[i:i + 1], w), (k, d, n, name, i, what)
            assert not torch.isnan(got[0]).any(), (k, d, n, name)
            nonzero += bool(got[0].abs().max() > 0)
        assert nonzero >= 4, (k, d, n, nonzero)  # (the windows are not all empty)


@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("k,d", LAYERS)
def test_mixed_table(k, d, poison, device):
    """Items at different positions in one launch, a paused and a fresh paused one among them."""
    for n in (5, 33, 70):
        case = _Layer(k, d, n, 6, device, 57 + n)
        items = [(0, None), (19, None), (FAR, None), (3, None), (FAR, -18), (0, None)]
        paused = {3: False, 5: True}  # item -> is it fresh
        rows = [_row(b, left, i in paused) for i, (b, left) in enumerate(items)]
        # what a fresh item must not read, and what a paused one must not read, holds NaN
        x, hist = case.x.clone(), case.hist.clone()
        for i in paused:
            x[i] = float("nan")
        for i in (0, 5):
            hist[i] = float("nan")
        got = case.slotted(rows, x, hist)
        if poison:
            with poison_lds():
                again = case.slotted(rows, x, hist)
            for g, a in zip(got, again):
                assert torch.equal(g, a), (k, d, n)
            continue
        for i, (before, left) in enumerate(items):
            if i in paused:
                assert torch.equal(got[0][i], torch.zeros_like(got[0][i])), (k, d, n, i)
                assert torch.equal(got[1][i], torch.zeros_like(got[1][i]) if paused[i] else case.hist[i]), (k, d, n, i)
                continue
            for g, w, what in zip(got, case.mirrored(i, before, left), ("y", "hist_out")):
                assert torch.equal(g[i:i + 1], w), (k, d, n, i, what)


# ---- 2. the slotted PQMF synthesis -----------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [False, True])
def test_slotted_pqmf_equals_the_stream_synthesis_of_its_items(poison, device):
    pq = layers.PQMF(4).to(device)
    h_cols, delay = pq.stream_history_columns, pq.stream_delay_columns
    assert (h_cols, delay) == (15, 8)
    for n in (6, 16, 70):  # (6 < H: part of the history carries over)
        gen = torch.Generator().manual_seed(300 + n)
        y = torch.randn(5, 4, n, generator=gen).to(device)
        hist = torch.randn(5, 4, h_cols, generator=gen).to(device)
        # items: running, fresh, paused, fresh and paused, running
        rows = [_row(7, None), _row(0, None), _row(7, None, True), _row(0, None, True), _row(FAR, -3)]
        y_in, hist_in = y.clone(), hist.clone()
        y_in[2], y_in[3], hist_in[1], hist_in[3] = float("nan"), float("nan"), float("nan"), float("nan")
        table = torch.tensor(rows, dtype=torch.int32, device=device)
        hist_out = _nan(device, 5, 4, h_cols)
        if poison:
            with poison_lds():
                x = pq.stream_synthesis_slots(y_in, hist_in, hist_out, table)
        else:
            x = pq.stream_synthesis_slots(y_in, hist_in, hist_out, table)
        assert x.shape == (5, 4 * n)
        for i, fresh in ((0, False), (1, True), (4, False)):
            ho = _nan(device, 1, 4, h_cols)
            h_i = torch.zeros(1, 4, h_cols, device=device) if fresh else hist[i:i + 1].contiguous()
            want = pq.stream_synthesis(y[i:i + 1].contiguous(), h_i, ho, n)
            assert torch.equal(x[i:i + 1], want) and torch.equal(hist_out[i:i + 1], ho), (n, i)
            # float64: the whole-signal synthesis of concat(history, chunk); the chunk positions [-D, n - D) of it
            window = torch.cat([h_i, y[i:i + 1]], -1).double().cpu()
            hs, ud = pq.synthesis_filter.double().cpu(), pq.updown_filter.double().cpu()
            ref = F.conv1d(F.pad(F.conv_transpose1d(window, ud * 4, stride=4), (31, 31)), hs)[:, 0]
            ref = ref[:, (h_cols - delay) * 4:(h_cols - delay + n) * 4]
            err = max_abs(x[i:i + 1], ref)
            print(f"slotted pqmf n={n} item {i} err {err:.3g}")
            assert err <= 2e-6 * max(1.0, ref.abs().max().item())  # tests/test_stream_mb_gpu.py: the stream kernel's bar
        for i, fresh in ((2, False), (3, True)):
            assert torch.equal(x[i], torch.zeros_like(x[i])), (n, i)
            assert torch.equal(hist_out[i], torch.zeros_like(hist[i]) if fresh else hist[i]), (n, i)


# ---- 3. the buffer checks --------------------------------------------------------------------------------------------
def test_slotted_mirrored_forward_checks_its_buffers(device):
    cv = layers.Conv1d(24, 40, 7, padding=3, pad_mode="reflect").to(device)
    x = torch.zeros(1, 24, 4, device=device)
    hist = [torch.zeros(1, 24, 6, device=device) for _ in range(2)]
    table = torch.zeros(1, ops.SLOT_INTS, dtype=torch.int32, device=device)
    desc, w = mirrored_desc(cv, 1, 4), cv.packed_weight()
    with pytest.raises(RuntimeError, match="hist_in is NULL"):
        ops.conv1d_stream_slots_mirrored_forward(desc, x, None, hist[1], w, slots=table, delay=3)
    with pytest.raises(RuntimeError, match="slots is NULL"):
        ops.conv1d_stream_slots_mirrored_forward(desc, x, hist[0], hist[1], w, delay=3)
    with pytest.raises(RuntimeError, match="pad_mode"):
        ops.conv1d_stream_slots_mirrored_forward(ops.make_conv_desc(1, 24, 40, 4, 4, 7, pad_left=6), x, hist[0], hist[1], w,
                                                 slots=table, delay=3)
    with pytest.raises(RuntimeError, match="distinct"):
        ops.conv1d_stream_slots_mirrored_forward(desc, x, hist[0], hist[0], w, slots=table, delay=3)
    with pytest.raises(RuntimeError, match="padding"):
        ops.conv1d_stream_slots_mirrored_forward(desc, x, hist[0], hist[1], w, slots=table, delay=2)
    pq = layers.PQMF(4).to(device)
    y, h = torch.zeros(1, 4, 8, device=device), [torch.zeros(pq.history_shape(1), device=device) for _ in range(2)]
    with pytest.raises(RuntimeError, match="hist_in is NULL"):
        pq.stream_synthesis_slots(y, None, h[1], table)
    with pytest.raises(RuntimeError, match="slots is NULL"):
        pq.stream_synthesis_slots(y, h[0], h[1], None)
    with pytest.raises(RuntimeError, match="distinct"):
        pq.stream_synthesis_slots(y, h[0], h[0], table)


# ---- 4. the pool -----------------------------------------------------------------------------------------------------
# the configs of tests/test_stream_melgan_lookahead_gpu.py, restated
TINY = dict(synth.MELGAN_CAUSAL, use_causal_conv=False)  # channels 64, scales [4, 2, 2], 2 stacks: 16 samples a frame
TINY_MB = dict(in_channels=80, out_channels=4, kernel_size=7, channels=32, upsample_scales=[3, 2], stack_kernel_size=3,
               stacks=3)  # an odd stride, dilations 1, 3, 9, 4 sub-bands: 24 samples a frame
CASES = {"tiny": (TINY, 90, 6, 16), "tiny_mb": (TINY_MB, 65 * 4 + 32, 13, 24)}  # cfg, latency, settle_frames, up
LENGTHS = (4, 5, 9, 14, 23)  # 4: min_frames; 23: past both settle counts; 5, 9, 14, 23: no multiples of the chunk
MB_G = dict(in_channels=80, out_channels=4, kernel_size=7, channels=384, upsample_scales=[8, 4, 2],
            stack_kernel_size=3, stacks=4, use_weight_norm=True, use_causal_conv=False)


@functools.lru_cache(maxsize=None)
def _utterances(name):
    """(state dict, [(T, 80) features on the CPU]): computed once, never modified."""
    sd = synth_for(models.MelGANGenerator(**CASES[name][0]), 21, synth.MELGAN_G_SCALE)
    return sd, [synth.synth_input(f"mpool{i}", (t, 80), seed=70 + i) for i, t in enumerate(LENGTHS)]


def _model(name, device):
    cfg = CASES[name][0]
    m = models.MelGANGenerator(**cfg)
    m.load_state_dict(_utterances(name)[0])
    m = m.to(device).eval()
    if cfg["out_channels"] > 1:
        m.pqmf = layers.PQMF(subbands=cfg["out_channels"]).to(device)
    return m


_REFERENCE = {}


def _reference(name, model):
    """Per utterance what ``MelGANLookaheadStream(batch=1)`` emits for it, pushes and flush together; once per case."""
    if name not in _REFERENCE:
        s, refs = MelGANLookaheadStream(model, batch=1, use_graph=False), []
        for f in _utterances(name)[1]:
            s.reset()
            refs.append(torch.cat([s.push(f[:2]), s.push(f[2:]), s.flush()], -1)[0])
        _REFERENCE[name] = refs
    return _REFERENCE[name]


def _drive(pool, feats):
    """All utterances through the pool: staggered ``open()``, irregular ``feed()`` sizes, slots reused (the pattern of
    tests/test_stream_pool_gpu.py) -> (per utterance the concatenated emissions, facts about the run)."""
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


@pytest.mark.parametrize("name", list(CASES))
def test_pool_equals_one_lookahead_stream_per_utterance(name, device):
    _, latency, settle, up = CASES[name]
    model, feats = _model(name, device), _utterances(name)[1]
    refs = _reference(name, model)
    pool = MelGANStreamPool(model, slots=3, chunk_frames=4, use_graph=False)
    assert (pool.latency_samples, pool.settle_frames, pool.min_frames, pool.up, pool.precision) == \
        (latency, settle, 4, up, "fp32")
    assert pool.state_bytes == 2 * 4 * sum(t.numel() for t in pool._halves[0]) == MelGANStreamPool.state_bytes_of(model, 3)
    got, facts = _drive(pool, feats)
    print("melgan pool", name, facts)
    assert facts["pauses"] > 0 and facts["reused"] > 0
    worst = 0.0
    for i, (y, ref) in enumerate(zip(got, refs)):
        assert y.shape == (LENGTHS[i] * up,) and torch.equal(y, ref), (name, i)
        with torch.no_grad():
            full = model(feats[i].t().unsqueeze(0).contiguous().to(device))
            full = (model.pqmf.synthesis(full) if model.pqmf is not None else full)[0, 0]
        worst = max(worst, max_abs(y, full))
    print("melgan pool", name, "against forward", worst)
    assert worst <= FORWARD_TOL
    # graph mode: one pair of graphs from the first step on, the same bits
    graphed = MelGANStreamPool(model, slots=3, chunk_frames=4, use_graph=True)
    assert graphed.graphs_captured == 0
    again, facts = _drive(graphed, feats)
    assert graphed.graphs_captured == 2 and facts["steps"] > 10
    for i, (y, ref) in enumerate(zip(again, refs)):
        assert torch.equal(y, ref), (name, i)
    # a second round in the same pool: every slot is reused
    assert all(torch.equal(y, ref) for y, ref in zip(_drive(graphed, feats)[0], refs)) and graphed.graphs_captured == 2


def test_pool_normalizes_and_pads_after_normalisation(device):
    model = _model("tiny_mb", device)
    gen = torch.Generator().manual_seed(17)
    mean, scale = torch.randn(80, generator=gen) * 0.1, 1.0 + 0.1 * torch.rand(80, generator=gen)
    model.register_buffer("mean", mean.to(device))
    model.register_buffer("scale", scale.to(device))
    f = torch.randn(9, 80, generator=gen) * scale + mean
    s = MelGANLookaheadStream(model, normalize_before=True, use_graph=False)
    ref = torch.cat([s.push(f), s.flush()], -1)[0]
    for graph in (False, True):
        pool = MelGANStreamPool(model, slots=2, chunk_frames=4, normalize_before=True, use_graph=graph)
        slot = pool.open()
        pool.feed(slot, f)
        pool.end(slot)
        outs = []
        while pool.open_slots:
            outs.append(pool.step()[slot])
        assert torch.equal(torch.cat(outs), ref), graph


@pytest.mark.parametrize("name", list(CASES))
def test_a_step_is_one_slotted_launch_per_plan_entry(name, device):
    model, feats = _model(name, device), _utterances(name)[1]
    pool = MelGANStreamPool(model, slots=3, chunk_frames=4, use_graph=False)
    a, b = pool.open(), pool.open()
    pool.feed(a, feats[2])
    pool.feed(b, feats[1][:2])  # paused
    pool.step()                 # (packs the weight images)
    with ops.profile() as prof:
        out = pool.step()
    assert list(out) == [a]
    plan = model.lookahead_plan()
    mirrored = sum(launch_is_mirrored(launch) for launch in plan)
    want = {"conv1d_stream_slots_kernel": len(plan) - mirrored, "conv1d_stream_slots_mirrored_kernel": mirrored}
    if model.pqmf is not None:
        want["pqmf_up_stream_slots_kernel"] = 1
    assert {k: v["launches"] for k, v in prof.results.items() if "stream" in k} == want
    # nothing to run: nothing is launched
    pool.end(a)
    while a in pool.open_slots:
        pool.step()
    with ops.profile() as prof:
        assert pool.step() == {}
    assert not prof.results


def test_an_utterance_too_short_for_reflection_closes_its_slot(device):
    model, feats = _model("tiny", device), _utterances("tiny")[1]
    refs = _reference("tiny", model)
    pool = MelGANStreamPool(model, slots=2, chunk_frames=4, use_graph=False)
    a, b = pool.open(), pool.open()
    pool.feed(a, feats[2])
    pool.feed(b, feats[3][:3])
    outs = [pool.step()[a]]
    with pytest.raises(RuntimeError, match="at least 4"):
        pool.end(b)
    assert pool.open_slots == [a]
    # the slot is free again and starts the next utterance fresh; the other slot's bits are unaffected
    assert pool.open() == b
    pool.feed(b, feats[1])
    pool.end(a)
    pool.end(b)
    outs_b = []
    while pool.open_slots:
        out = pool.step()
        outs += [out[a]] if a in out else []
        outs_b += [out[b]] if b in out else []
    assert torch.equal(torch.cat(outs), refs[2]) and torch.equal(torch.cat(outs_b), refs[1])


def test_multi_band_golden_through_the_pool(device):
    gold = load_golden("mb_melgan_v2")
    seed = int(gold["meta"][0])
    g = models.MelGANGenerator(**MB_G)
    g.load_state_dict(synth.synth_state_dict(g.state_dict(), seed=seed, g_scale=synth.MELGAN_G_SCALE))
    g = g.to(device).eval()
    g.pqmf = layers.PQMF().to(device)
    f = synth.synth_input("c", (2, 80, 24), seed=seed)[0].t().contiguous()  # (24, 80)
    pool = MelGANStreamPool(g, slots=2, chunk_frames=8, use_graph=False)
    assert (pool.latency_samples, pool.up) == (672 * 4 + 32, 256)
    slot, outs, t = pool.open(), [], 0
    for n in (5, 7, 1, 11):
        pool.feed(slot, f[t:t + n])
        t += n
        out = pool.step()
        outs += [out[slot]] if slot in out else []
    pool.end(slot)
    while pool.open_slots:
        outs.append(pool.step()[slot])
    y = torch.cat(outs)
    err = max_abs(y, gold["g_y_inference"].reshape(-1))
    print("mb_melgan_v2 golden through the pool", err)
    assert y.shape == (24 * 256,) and err <= WAVE_TOL
