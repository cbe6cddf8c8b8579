"""CPU: host logic of the Parallel WaveGAN stream pool (utils.PWGStreamPool) -- the slotted walk, the
second table's windows, what a tail or drain chunk holds, the entry points, the state's size and what the pool refuses.
Nothing here launches a kernel."""
import ctypes
import itertools

import pytest
import torch

from parallelwavegan_amd import _lib, models, ops
from parallelwavegan_amd.layers.causal_conv import (PWGLookaheadWalk, PWGSlotWalk, SlotPosition, pwg_lookahead_state_shapes,
                                                    slot_table_rows_in)
from parallelwavegan_amd.utils import PWGStreamPool, StreamPool, set_inference_precision
from parallelwavegan_amd.utils.streaming import SlotSchedule, slot_window
from tests.golden import synth

SMALL = dict(layers=6, stacks=2, aux_context_window=2, upsample_params={"upsample_scales": [4, 4]})  # latency 66, up 16


# ---- the walk --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [SMALL, {}, dict(SMALL, aux_context_window=0)])
def test_slot_walk_hands_out_the_table_where_the_lock_step_walk_hands_out_the_window(cfg):
    """``PWGSlotWalk.take`` against the plan: the launches in order, the same state pairs as ``PWGLookaheadWalk``, and the
    table, rate and delay in the window's place; ``conv_in`` with a history gets the second table and ``delay + rate``."""
    g = models.ParallelWaveGANGenerator(**cfg)
    plan = g.lookahead_plan()
    shapes = pwg_lookahead_state_shapes(plan, 3)
    halves = [[object() for _ in shapes] for _ in range(2)]
    first, second = object(), object()
    slotted = PWGSlotWalk(plan, halves[0], halves[1], first, second, "bf16")
    lock = PWGLookaheadWalk(plan, halves[0], halves[1], 5, None, "bf16")
    assert slotted.precision == "bf16" and not slotted.at_start
    at = 0
    for launch in plan:
        got, pairs, where = slotted.take(launch.kind, launch.module, 4)
        _, want_pairs, valid = lock.take(launch.kind, launch.module, 4)
        assert got is launch and pairs == want_pairs == list(zip(halves[0][at:at + len(launch.state)],
                                                                   halves[1][at:at + len(launch.state)]))
        at += len(launch.state)
        assert isinstance(where, SlotPosition) and isinstance(valid, tuple)
        if launch.kind == "conv_in" and launch.state:
            assert where == SlotPosition(second, 1, launch.delay + 1, first)
        else:
            assert where == SlotPosition(first, launch.rate, launch.delay, None)
    assert at == len(shapes)
    with pytest.raises(StopIteration):
        slotted.take("layer", None, 4)
    # out of step, no start-of-stream form, the second table where conv_in keeps a history
    with pytest.raises(RuntimeError, match="out of step"):
        PWGSlotWalk(plan, halves[0], halves[1], first, second).take("layer", None, 4)
    with pytest.raises(ValueError, match="state_in"):
        PWGSlotWalk(plan, None, halves[1], first)
    with pytest.raises(ValueError, match="precision"):
        PWGSlotWalk(plan, halves[0], halves[1], first, precision="fp16")
    if plan[0].kind == "conv_in" and plan[0].state:
        with pytest.raises(RuntimeError, match="second table"):
            PWGSlotWalk(plan, halves[0], halves[1], first).take("conv_in", plan[0].module, 4)
    else:
        assert PWGSlotWalk(plan, halves[0], halves[1], first).take(plan[0].kind, plan[0].module, 4)[2].slots is first


# ---- the second table ------------------------------------------------------------------------------------------------
def test_second_table_gives_the_first_tables_windows_on_a_small_grid():
    """``conv_in`` runs with ``delay + rate`` over rows ``(before + 1, left - 1, flags)``: the windows of ``delay`` over the
    first table, on the exhaustive grid of tests/test_stream_pool_host.py, and no row of it is fresh."""
    n = 0
    for delay, rate, chunk, before in itertools.product((0, 1, 3, 7, 14), (1, 2, 4), (1, 2, 5), range(0, 9)):
        t_out = chunk * rate
        for left in [None] + list(range(-8, 9)):
            flags = 0 if left is None else ops.SLOT_LEFT_KNOWN
            ((b2, l2, f2, own),) = slot_table_rows_in([(before, left or 0, flags, 7)])
            assert (f2, own) == (flags, 7) and b2 >= 1
            assert slot_window(delay + rate, rate, t_out, b2, None if left is None else l2) == \
                slot_window(delay, rate, t_out, before, left), (delay, rate, t_out, before, left)
            n += 1
    assert n > 5000


def test_second_table_near_2_to_the_31_frames():
    big = 2 ** 31 - 1
    for before in (big - 3, big - 1):  # (before + 1 still fits the table's int32; the schedule saturates long before)
        for left in (-3, 0, 2, 5):
            ((b2, l2, _, _),) = slot_table_rows_in([(before, left, ops.SLOT_LEFT_KNOWN, 0)])
            assert b2 <= big
            assert slot_window(2 + 1, 1, 8, b2, l2) == slot_window(2, 1, 8, before, left) == (0, min(max(2 + left, 0), 8))
    # what the schedule really writes: the position saturated at settle, the frames left at [-settle, chunk]
    sch = SlotSchedule(1, 4, 16, 66, 5)
    s = sch.open()
    sch.feed(s, 9)
    sch.end(s)
    rows = []
    while s in sch.open_slots:
        rows.append(sch.advance()[0].row)
    assert [r[:2] for r in rows] == [(0, 4), (4, 4), (5, 1), (5, -3)]
    for (before, left, flags, _), (b2, l2, f2, _) in zip(rows, slot_table_rows_in(rows)):
        assert (b2, l2, f2) == (before + 1, left - 1, flags)


# ---- what a step uploads ---------------------------------------------------------------------------------------------
def _host_pool(slots, chunk, up, latency, two_tables=True):
    """A pool's host side without its device side: the schedule, the queues and ``_fill``."""
    pool = object.__new__(PWGStreamPool)
    pool.slots = pool.batch = slots
    pool.chunk_frames, pool.up, pool._two_tables = chunk, up, two_tables
    pool._schedule = SlotSchedule(slots, chunk, up, latency, -(-latency // up))
    pool._feats = torch.zeros(slots, chunk, 80)
    pool.frames_in = 0
    pool._queues = [[] for _ in range(slots)]
    pool._noise_queues = [[] for _ in range(slots)]
    pool._last = [None] * slots
    return pool


def test_tail_and_drain_chunks_replicate_the_last_frame_with_zero_noise():
    chunk, up = 4, 16
    pool = _host_pool(2, chunk, up, 66)
    gen = torch.Generator().manual_seed(1)
    f, z = torch.randn(6, 80, generator=gen), torch.randn(6 * up, generator=gen)
    a, b = pool.open(), pool.open()
    pool.feed(a, f[:5], z[:5 * up])
    pool.feed(a, f[5:])  # one frame whose noise is drawn later: NaN on the host
    pool.feed(b, f[:2], z[:2 * up])
    pool.end(a)
    table, feats, noise = torch.zeros(4, 4, dtype=torch.int32), torch.full((2, chunk, 80), 9.0), torch.full((2, 1, chunk * up), 9.0)
    kept_b = (feats[b].clone(), noise[b].clone())
    # step 1: a full chunk of a; b is paused and its staging rows are left alone
    steps = pool._schedule.advance()
    pool._fill(steps, table, feats, noise)
    assert [st.action for st in steps] == ["run", "pause"]
    assert torch.equal(feats[a], f[:4]) and torch.equal(noise[a, 0], z[:4 * up])
    assert torch.equal(feats[b], kept_b[0]) and torch.equal(noise[b], kept_b[1])
    assert table[:2].tolist() == [list(st.row) for st in steps] and table[a, 3].item() == 4
    assert table[2:].tolist() == [[r[0] + 1, r[1] - 1, r[2], r[3]] for r in table[:2].tolist()]
    # step 2: a's tail -- two real frames, then copies of the last one; the drawn frame's noise is NaN, the padding's zero
    steps = pool._schedule.advance()
    pool._fill(steps, table, feats, noise)
    assert steps[a].action == "tail" and table[a].tolist() == [4, 2, ops.SLOT_LEFT_KNOWN, 2]
    assert torch.equal(feats[a, :2], f[4:6]) and torch.equal(feats[a, 2:], f[5].expand(2, -1))
    assert torch.equal(noise[a, 0, :up], z[4 * up:5 * up]) and torch.isnan(noise[a, 0, up:2 * up]).all()
    assert torch.equal(noise[a, 0, 2 * up:], torch.zeros(2 * up))
    # then drain chunks: the last frame throughout, zero noise, no real frames (row[3] == 0)
    while a in pool.open_slots:
        steps = pool._schedule.advance()
        pool._fill(steps, table, feats, noise)
        assert steps[a].action == "drain" and table[a, 3].item() == 0
        assert torch.equal(feats[a], f[5].expand(chunk, -1)) and torch.equal(noise[a, 0], torch.zeros(chunk * up))
    # the slot's next utterance keeps nothing of the last one
    assert pool.open() == a
    pool.feed(a, f[:1], z[:up])
    pool.end(a)
    pool._fill(pool._schedule.advance(), table, feats, noise)
    assert torch.equal(feats[a], f[0].expand(chunk, -1)) and torch.equal(noise[a, 0, up:], torch.zeros(3 * up))
    # what feed refuses
    with pytest.raises(ValueError, match="noise"):
        pool.feed(b, f[:1], z[:3])
    with pytest.raises(ValueError, match="finite"):
        pool.feed(b, f[:1], torch.full((up,), float("nan")))
    with pytest.raises(ValueError, match="features"):
        pool.feed(b, f[:1, :79])


def test_one_table_without_a_context_window():
    pool = _host_pool(1, 4, 16, 48, two_tables=False)
    s = pool.open()
    pool.feed(s, torch.ones(4, 80))
    table = torch.zeros(1, 4, dtype=torch.int32)
    pool._fill(pool._schedule.advance(), table, torch.zeros(1, 4, 80), torch.zeros(1, 1, 64))
    assert table.tolist() == [[0, 0, 0, 4]]


# ---- the entry points ------------------------------------------------------------------------------------------------
def test_slotted_entry_points_are_exported_under_the_same_abi():
    assert _lib.ABI_VERSION == _lib.lib().pwg_abi_version() == 15
    position = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]
    for name in ("pwg_wavenet_stream_slots_forward", "pwg_wavenet_stream_slots_forward_bf16", "pwg_stretch_conv_stream_slots",
                 "pwg_delay_line_slots_forward", "pwg_slot_seed_history"):
        assert name in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    # the arguments of the delayed entry points, the window replaced by (slots, rate, delay)
    res, args = _lib.SIGNATURES["pwg_wavenet_stream_delayed_forward"]
    assert _lib.SIGNATURES["pwg_wavenet_stream_slots_forward"] == (res, args[:15] + position + args[17:])
    res, args = _lib.SIGNATURES["pwg_wavenet_stream_bf16_delayed_forward"]
    assert _lib.SIGNATURES["pwg_wavenet_stream_slots_forward_bf16"] == (res, args[:15] + position + args[17:19] + args[21:])
    res, args = _lib.SIGNATURES["pwg_stretch_conv_stream_delayed"]  # rows -> items, channels
    assert _lib.SIGNATURES["pwg_stretch_conv_stream_slots"] == (res, args[:6] + [ctypes.c_int32] + args[6:11] + position
                                                                + args[13:])
    res, args = _lib.SIGNATURES["pwg_delay_line_forward"]
    assert _lib.SIGNATURES["pwg_delay_line_slots_forward"] == (res, args[:5] + [ctypes.c_int32] + args[5:7]
                                                               + [ctypes.c_void_p] + args[7:])


def test_slotted_wrappers_refuse_cpu_tensors():
    table = torch.zeros(1, ops.SLOT_INTS, dtype=torch.int32)
    x, h = torch.zeros(1, 3, 4), torch.zeros(1, 3, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.stretch_conv_stream_slots(x, h, h.clone(), torch.zeros(9), 4, slots=table)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.delay_line_slots_forward(x, h, h.clone(), table)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.slot_seed_history(x, h, table)


# ---- the state -------------------------------------------------------------------------------------------------------
def test_state_bytes_follow_the_plans_shapes():
    g = models.ParallelWaveGANGenerator(**SMALL)
    # per slot: conv_in 80 x 4, two stages 80 x 2, the noise line 1 x 52, the conditioning line 80 x sum(d), per layer
    # 64 x 2d and (from the second on) a skip line 64 x d; dilations 1, 2, 4 twice
    dil = [1, 2, 4, 1, 2, 4]
    per_slot = 80 * 4 + 2 * 80 * 2 + 52 + 80 * sum(dil) + sum(64 * 2 * d for d in dil) + sum(64 * d for d in dil[1:])
    assert g.lookahead_plan()[2].delay == 52  # (2 * 4 + 4) * 4 + 4
    assert PWGStreamPool.state_bytes_of(g, 3) == 2 * 4 * 3 * per_slot
    v1 = models.ParallelWaveGANGenerator()
    assert PWGStreamPool.state_bytes_of(v1, 16) == 16 * PWGStreamPool.state_bytes_of(v1, 1)


# ---- what the pool refuses -------------------------------------------------------------------------------------------
def test_pwg_stream_pool_refuses_models_it_cannot_stream():
    with pytest.raises(ValueError, match="utils.StreamPool"):
        PWGStreamPool(models.HiFiGANGenerator(**synth.HIFIGAN_TINY))
    with pytest.raises(ValueError, match="MelGANGenerator is not supported"):
        PWGStreamPool(models.MelGANGenerator(channels=64, upsample_scales=[4, 2, 2], stacks=2))
    with pytest.raises(ValueError, match="PWGStream"):
        PWGStreamPool(models.ParallelWaveGANGenerator(**synth.PWG_CAUSAL))
    with pytest.raises(ValueError, match="out_channels"):
        PWGStreamPool(models.ParallelWaveGANGenerator(**dict(SMALL, out_channels=2)))
    with pytest.raises(ValueError, match="only 64 / 128 / 64"):
        PWGStreamPool(models.ParallelWaveGANGenerator(**dict(SMALL, residual_channels=32)))
    g = models.ParallelWaveGANGenerator(**SMALL)
    set_inference_precision(g, "bf16")
    with pytest.raises(ValueError, match="bf16") as info:
        PWGStreamPool(g)
    assert "precision='bf16'" in str(info.value)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # (past every check of the model: the device check)
        PWGStreamPool(g, precision="bf16")
    g = models.ParallelWaveGANGenerator(**SMALL)
    with pytest.raises(ValueError, match="PWGStreamPool: slots"):
        PWGStreamPool(g, slots=0)
    with pytest.raises(ValueError, match="PWGStreamPool: chunk_frames"):
        PWGStreamPool(g, chunk_frames=0)
    with pytest.raises(ValueError, match="precision"):
        PWGStreamPool(g, precision="fp16")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PWGStreamPool(g)


def test_stream_pool_still_names_the_lock_step_stream():
    with pytest.raises(ValueError, match="a ParallelWaveGANGenerator through utils.PWGLookaheadStream"):
        StreamPool(models.ParallelWaveGANGenerator(**SMALL))
