"""CPU: host logic of the stream pool (utils.StreamPool, the slotted form of the streaming convolution, DESIGN.md
s11.10) -- the window rule, the schedule of the slots, the entry points and what the pool refuses.  Nothing here
launches a kernel."""
import ctypes
import itertools

import pytest
import torch

from parallelwavegan_amd import _lib, models, ops
from parallelwavegan_amd.layers.causal_conv import _STREAM_KERNELS, SlotWalk, lookahead_window
from parallelwavegan_amd.utils import LookaheadStream, StreamPool, set_inference_precision
from parallelwavegan_amd.utils.streaming import SlotSchedule, slot_window
from tests.golden import synth


# ---- the window rule -----------------------------------------------------------------------------------------------
def test_window_rule_equals_lookahead_window_on_a_small_grid():
    """``slot_window`` takes the frames LEFT where ``lookahead_window`` takes the total: every (delay, rate, t_out,
    frames before, frames left) of a small grid, with the end known and unknown, past the end included."""
    n = 0
    for delay, rate, chunk, before in itertools.product((0, 1, 3, 7, 14), (1, 2, 4), (1, 2, 5), range(0, 9)):
        t_out = chunk * rate
        assert slot_window(delay, rate, t_out, before) == lookahead_window(delay, rate, t_out, before, None)
        for left in range(-8, 9):
            if before + left < 0:  # (an utterance has no negative length)
                continue
            assert slot_window(delay, rate, t_out, before, left) == \
                lookahead_window(delay, rate, t_out, before, before + left), (delay, rate, t_out, before, left)
            n += 1
    assert n > 5000
    # steady state (``frames_before`` None there) is any position past the delay
    assert slot_window(14, 4, 20, 4) == lookahead_window(14, 4, 20) == (0, 20)


def test_window_rule_near_2_to_the_31_frames():
    big = 2 ** 31 - 1
    for before in (big - 3, big, 2 ** 31 + 5, 2 ** 40):
        for left in (-3, 0, 2, 5):
            assert slot_window(3258, 256, 2048, before, left) == \
                lookahead_window(3258, 256, 2048, before, before + left) == (0, min(max(3258 + 256 * left, 0), 2048))


def test_saturated_positions_give_the_same_windows():
    """What ``SlotSchedule`` puts into the table -- the position capped at ``settle``, the frames left clamped to
    ``[-settle, chunk]`` -- gives the window of the true numbers, for every launch of the plan."""
    g = models.HiFiGANGenerator(**synth.HIFIGAN_TINY)
    plan, chunk = g.lookahead_plan(), 4
    settle = max(-(-launch.delay // launch.rate) for launch in plan)
    for launch in plan:
        t_out = chunk * launch.rate
        for before in (0, 1, settle - 1, settle, settle + 1, 10 ** 12):
            for left in (None, -10 ** 12, -settle - 1, -settle, -1, 0, 1, chunk, chunk + 1, 10 ** 12):
                sat = None if left is None else max(-settle, min(left, chunk))
                assert slot_window(launch.delay, launch.rate, t_out, min(before, settle), sat) == \
                    slot_window(launch.delay, launch.rate, t_out, before, left), (launch[1:], before, left)


# ---- the schedule --------------------------------------------------------------------------------------------------
UP, LATENCY, SETTLE, CHUNK = 24, 182, 8, 4  # the tiny generator: 182 samples = 7.6 frames


def _emitted(frames_in, total=None):
    """``_LookaheadStream``'s arithmetic: the emissions after ``frames_in`` frames went in."""
    n = max(0, frames_in * UP - LATENCY)
    return n if total is None else min(n, total * UP)


def test_schedule_scenario():
    sch = SlotSchedule(3, CHUNK, UP, LATENCY, SETTLE)
    assert sch.advance() == [] and sch.open_slots == []
    a, b = sch.open(), sch.open()
    assert (a, b) == (0, 1)
    sch.feed(a, 5)
    sch.feed(b, 3)
    assert sch.open_slots == [0, 1]
    # step 1: a runs on 4 of its 5 frames, b is paused (fresh), slot 2 is empty (fresh and paused)
    s = sch.advance()
    assert [(x.action, x.take, x.row) for x in s] == [("run", 4, (0, 0, 0, 4)), ("pause", 0, (0, 0, ops.SLOT_PAUSED, 0)),
                                                      ("empty", 0, (0, 0, ops.SLOT_PAUSED, 0))]
    assert s[0].emit[1] - s[0].emit[0] == 0 and not s[0].closes
    # nothing to run: a has one frame, b three
    assert sch.advance() == []
    # b ends after 3 frames: its tail runs padded, with the remaining length known; a still waits
    sch.end(b)
    s = sch.advance()
    assert (s[0].action, s[0].row) == ("pause", (4, 0, ops.SLOT_PAUSED, 0))
    assert (s[1].action, s[1].take, s[1].row) == ("tail", 3, (0, 3, ops.SLOT_LEFT_KNOWN, 3))
    with pytest.raises(RuntimeError, match="ended"):
        sch.feed(b, 1)
    # b drains on zero chunks until its 3 * 24 samples are out, then closes
    got, steps = 0, 1
    while b in sch.open_slots:
        s = sch.advance()
        steps += 1
        assert s[1].action == "drain" and s[1].take == 0 and s[1].row[2] == ops.SLOT_LEFT_KNOWN
        assert s[1].row[0] == min(4 * (steps - 1), SETTLE) and s[1].row[1] == max(3 - 4 * (steps - 1), -SETTLE)
        got += s[1].emit[1] - s[1].emit[0]
        assert got == _emitted(4 * steps, 3)
        lo, hi = s[1].emit
        assert 0 <= lo <= hi <= CHUNK * UP
    assert got == 3 * UP and steps == 3  # ceil((72 + 182) / 96)
    # the slot is free again and the next utterance in it starts fresh
    assert sch.open() == b
    sch.feed(b, 4)
    sch.feed(a, 3)
    s = sch.advance()
    assert (s[0].action, s[0].row) == ("run", (4, 0, 0, 4)) and (s[1].action, s[1].row) == ("run", (0, 0, 0, 4))
    with pytest.raises(RuntimeError, match="not open"):
        sch.feed(2, 1)
    # an empty utterance closes at once; a full pool refuses
    c = sch.open()
    sch.end(c)
    assert c not in sch.open_slots
    assert sch.open() == c
    with pytest.raises(RuntimeError, match="slots are taken"):
        sch.open()


@pytest.mark.parametrize("frames", [1, 3, 4, 9, 23])
def test_schedule_emission_totals_follow_the_lookahead_stream(frames):
    """One utterance fed in irregular pieces: after every step the emissions total ``clamp(frames_in * up - latency, 0,
    frames * up)``, every emitted range lies inside the step's output, and the position in the table saturates."""
    sch = SlotSchedule(1, CHUNK, UP, LATENCY, SETTLE)
    s = sch.open()
    fed, got, taken = 0, 0, 0
    pieces = itertools.cycle((1, 0, 2, 5))
    while s in sch.open_slots:
        if fed < frames:
            n = min(next(pieces), frames - fed)
            sch.feed(s, n)
            fed += n
            if fed == frames:
                sch.end(s)
        step = sch.advance()
        if not step:
            continue
        (st,) = step
        assert st.row[0] == min(taken, SETTLE)
        taken += CHUNK
        lo, hi = st.emit
        got += hi - lo
        assert got == _emitted(taken, frames if fed == frames else None)
        assert hi == lo or 0 <= lo < hi <= CHUNK * UP
    assert got == frames * UP


# ---- the entry points ----------------------------------------------------------------------------------------------
def test_slotted_entry_points_are_exported_under_the_same_abi():
    assert _lib.ABI_VERSION == _lib.lib().pwg_abi_version() == 15
    for name in ("pwg_conv1d_stream_slots_forward", "pwg_conv1d_stream_slots_forward_bf16"):
        assert name in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    # the arguments of the delayed entry points, the window replaced by (slots, rate, delay)
    for slotted, delayed in (("pwg_conv1d_stream_slots_forward", "pwg_conv1d_stream_delayed_forward"),
                             ("pwg_conv1d_stream_slots_forward_bf16", "pwg_conv1d_stream_bf16_delayed_forward")):
        res, args = _lib.SIGNATURES[delayed]
        assert _lib.SIGNATURES[slotted] == (res, args[:14] + [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32] + args[16:])
    assert _STREAM_KERNELS["slots", "fp32"][1:] == (ops.conv1d_stream_delayed_supported, ops.conv1d_stream_slots_forward)
    assert _STREAM_KERNELS["slots", "bf16"][1:] == (ops.conv1d_stream_bf16_delayed_supported,
                                                    ops.conv1d_stream_slots_forward_bf16)


def test_slotted_forward_refuses_cpu_tensors():
    d = ops.make_conv_desc(1, 4, 4, 8, 8, 3, pad_left=2)
    table = torch.zeros(1, ops.SLOT_INTS, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.conv1d_stream_slots_forward(d, torch.zeros(1, 4, 8), torch.zeros(1, 4, 2), torch.zeros(1, 4, 2),
                                        torch.zeros(3 * 16 * 128), slots=table)
    image = torch.zeros(_lib.lib().pwg_conv1d_bf16_packed_weight_bytes(ctypes.byref(d)), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="device image"):
        ops.conv1d_stream_slots_forward_bf16(d, torch.zeros(1, 4, 8), torch.zeros(1, 4, 2), torch.zeros(1, 4, 2), image,
                                             slots=table)


def test_slot_walk_has_no_start_of_stream_form():
    with pytest.raises(ValueError, match="state_in"):
        SlotWalk([], None, [], None)
    with pytest.raises(ValueError, match="precision"):
        SlotWalk([], [], [], None, precision="fp16")


# ---- what the pool refuses -----------------------------------------------------------------------------------------
def test_stream_pool_refuses_models_it_cannot_stream():
    with pytest.raises(ValueError, match="CausalStream"):
        StreamPool(models.HiFiGANGenerator(**synth.HIFIGAN_CAUSAL))
    with pytest.raises(ValueError, match="MelGANLookaheadStream"):
        StreamPool(models.MelGANGenerator(channels=64, upsample_scales=[4, 2, 2], stacks=2))
    with pytest.raises(ValueError, match="PWGLookaheadStream"):
        StreamPool(models.ParallelWaveGANGenerator(layers=4, stacks=2, upsample_params={"upsample_scales": [4, 4]}))
    with pytest.raises(ValueError, match="out_channels"):
        StreamPool(models.HiFiGANGenerator(**dict(synth.HIFIGAN_TINY, out_channels=4)))
    g = models.HiFiGANGenerator(**synth.HIFIGAN_TINY)
    set_inference_precision(g, "bf16")
    with pytest.raises(ValueError, match="bf16") as info:
        StreamPool(g)
    assert "precision='bf16'" in str(info.value)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # (past every check of the model: the device check)
        StreamPool(g, precision="bf16")
    g = models.HiFiGANGenerator(**synth.HIFIGAN_TINY)
    with pytest.raises(ValueError, match="slots"):
        StreamPool(g, slots=0)
    with pytest.raises(ValueError, match="chunk_frames"):
        StreamPool(g, chunk_frames=0)
    with pytest.raises(ValueError, match="precision"):
        StreamPool(g, precision="fp16")
    with pytest.raises(ValueError, match="non-decreasing"):
        StreamPool(models.HiFiGANGenerator(**dict(synth.HIFIGAN_TINY, resblock_kernel_sizes=(7, 3))))
    with pytest.raises(ValueError, match="LDS"):
        StreamPool(models.HiFiGANGenerator(**dict(synth.HIFIGAN_TINY, resblock_kernel_sizes=(11,),
                                                  resblock_dilations=[(1, 15)])))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        StreamPool(g)


def test_pool_latency_is_the_lookahead_streams():
    g = models.HiFiGANGenerator(**synth.HIFIGAN_TINY)
    assert LookaheadStream.latency_samples_of(g) == g.lookahead_plan()[-1].delay == LATENCY
