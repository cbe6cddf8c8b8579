"""Host logic of the chained block of split-operand units (resblock_split_kernel, csrc/resunit_split.hip; DESIGN.md
s9.2, "The chained block"): what the kernel covers, its frame, the admission predicate and the join rule of
``HiFiGANResidualBlock.forward``.  No device is needed."""
import pytest
import torch

from parallelwavegan_amd import _lib, ops
from parallelwavegan_amd.layers import conv as conv_mod
from parallelwavegan_amd.layers.conv import resblock_split_admitted

DILATIONS = (1, 3, 5)


def _desc(c, k, t=1000, pair=True, b=2):
    return ops.make_resunit_desc(b, c, t, k, 1, pair)


def _reason():
    return _lib.lib().pwg_last_error().decode()


def test_supported_answers_and_reasons():
    for c, k, n in [(32, 3, 3), (32, 3, 2), (32, 7, 3), (32, 11, 3), (64, 3, 3), (64, 3, 2), (64, 7, 2), (32, 3, 1)]:
        assert ops.resblock_split_supported(_desc(c, k), DILATIONS[:n]), (c, k, n, _reason())
    # fewer than half of the frame's columns stored: the 64-channel k = 7 / 11 blocks (56 and 8 of 128)
    assert not ops.resblock_split_supported(_desc(64, 7), DILATIONS)
    assert "56 outputs per frame of 128" in _reason()
    assert not ops.resblock_split_supported(_desc(64, 11), DILATIONS)
    assert "8 outputs per frame of 128" in _reason()
    # a single-convolution unit
    assert not ops.resblock_split_supported(_desc(32, 3, pair=False), DILATIONS)
    assert "single-convolution" in _reason()
    # the unit count
    assert not ops.resblock_split_supported(_desc(32, 3), (1, 3, 5, 7))
    assert "n_units" in _reason()
    assert not ops.resblock_split_supported(_desc(32, 3), ())
    # whatever the unit refuses: channels, T % 4, an even kernel, a dilation
    assert not ops.resblock_split_supported(_desc(128, 3), DILATIONS) and "channels" in _reason()
    assert not ops.resblock_split_supported(_desc(32, 3, t=66), DILATIONS) and "multiple of 4" in _reason()
    assert not ops.resblock_split_supported(_desc(32, 4), DILATIONS) and "odd" in _reason()
    assert not ops.resblock_split_supported(_desc(32, 3), (1, 0, 5)) and "dilation" in _reason()
    assert not ops.resblock_split_supported(_desc(32, 3), (1, 3, 60)) and "LDS" in _reason()


@pytest.mark.parametrize("c", (32, 64))
@pytest.mark.parametrize("k", (3, 7, 11))
@pytest.mark.parametrize("n", (1, 2, 3))
def test_frame_follows_the_definition(c, k, n):
    """Validity shrinks by (k - 1) / 2 * (d_u + 1) columns per unit and side; the frame's origin t0 - edge is kept a
    multiple of 4, so the sum is rounded up to one (it is one already for N = 3 at every k)."""
    H, p, dil = (256 if c == 32 else 128), (k - 1) // 2, DILATIONS[:n]
    shrink = sum(p * (d + 1) for d in dil)
    edge = (shrink + 3) // 4 * 4
    if n == 3:
        assert edge == shrink
    desc = _desc(c, k)
    if H - 2 * edge < H // 2:
        assert not ops.resblock_split_supported(desc, dil)
        return
    f = ops.resblock_split_frame(desc, dil)
    assert f["H"] == H and f["edge"] == edge and f["bn_out"] == H - 2 * edge, f
    assert f["edge"] % 4 == 0 and f["bn_out"] % 4 == 0  # frame t starts at t * bn_out - edge: a multiple of 4
    assert f["margin"] == p * max(dil) and f["lds"] == 3 * (H + 2 * f["margin"]) * (c + 8) * 2 <= 80 * 1024
    assert f["tiles"] == -(-desc.t // f["bn_out"])
    if (k, n) == (3, 3):
        assert f["bn_out"] == (232 if c == 32 else 104) and f["lds"] <= 64 * 1024
    if (c, k, n) == (32, 7, 3):
        assert f["bn_out"] == 184


def test_admission_predicate(monkeypatch):
    monkeypatch.setattr(conv_mod, "RESBLOCK_SPLIT_ADMITTED", {(32, 3): (3, 1000)})
    assert resblock_split_admitted(32, 3, 3, 1000, False)
    assert resblock_split_admitted(32, 3, 2, 1000, False)
    assert not resblock_split_admitted(32, 3, 3, 1000, False, enabled=False), "the switch is off"
    assert not resblock_split_admitted(32, 3, 3, 1000, True), "a gradient is needed"
    assert not resblock_split_admitted(32, 3, 3, 999, False), "below the column floor"
    assert not resblock_split_admitted(32, 7, 3, 1 << 20, False), "a class that is not listed"
    assert not resblock_split_admitted(32, 3, 4, 1 << 20, False), "more units than the row admits"
    assert not resblock_split_admitted(32, 3, 1, 1 << 20, False), "one unit is the unit kernel's"


def test_table_rows_stay_above_the_launches_other_tests_pin():
    """tests/test_hifigan_fewtap_split_gpu.py counts three unit launches at the unit table's floor, and
    tests/test_hifigan_resunit_split_gpu.py at 2 x 12800 columns."""
    for (c, k), (n, min_cols) in conv_mod.RESBLOCK_SPLIT_ADMITTED.items():
        unit = conv_mod.RESUNIT_SPLIT_ADMITTED[(c, k, True)]
        assert unit[0] == "unit" and 2 <= n <= 3
        assert min_cols > max(unit[1], 25600)
        assert ops.resblock_split_supported(_desc(c, k), DILATIONS[:n])


@pytest.fixture
def stub_block(monkeypatch):
    """A 3-unit block whose launches are recorded instead of run."""
    from parallelwavegan_amd.layers import HiFiGANResidualBlock
    from parallelwavegan_amd.layers import residual_block as rb

    events = []
    blk = HiFiGANResidualBlock(3, 32, DILATIONS)
    monkeypatch.setattr(conv_mod.Conv1d, "packed_weight_split", lambda self: "image", raising=False)

    def route(idx, x, accum, out_div):
        return "unit", ops.make_resunit_desc(x.shape[0], 32, x.shape[2], 3, DILATIONS[idx], True, 0.1, 0.1, out_div), None, None

    def block(desc, x, dilations, s1, s2, w1, b1, w2, b2, add2=None):
        events.append(("block", tuple(dilations), add2, desc.out_div))
        return x + len(dilations)

    def unit(idx, x, accum, out_div):
        events.append(("unit", idx, accum() if callable(accum) else accum, out_div))
        return x + 1

    monkeypatch.setattr(blk, "_unit_route", route)
    monkeypatch.setattr(blk, "_unit_one_launch", unit)
    monkeypatch.setattr(rb.ops, "resblock_split_supported", lambda d, dil: True)
    monkeypatch.setattr(rb.ops, "resblock_forward_split", block)
    monkeypatch.setattr(rb, "resblock_split_admitted", lambda c, k, n, cols, grad, enabled=True: enabled)
    return blk, events


def test_forward_fuses_the_whole_block_without_a_join(stub_block):
    blk, events = stub_block
    x, addend = torch.zeros(2, 32, 64), torch.ones(2, 32, 64)
    with torch.no_grad():
        y = blk(x, accum=addend, out_div=3.0)
    assert events == [("block", DILATIONS, addend, 3.0)] and float(y[0, 0, 0]) == 3.0


def test_forward_keeps_a_pending_join_in_front_of_the_last_unit(stub_block):
    """The previous MRF branch is waited for only in front of the block's last kernel: N - 1 units fuse, the last runs
    as it does today and resolves the join."""
    blk, events = stub_block
    x, addend = torch.zeros(2, 32, 64), torch.ones(2, 32, 64)

    def join():
        events.append("join")
        return addend

    with torch.no_grad():
        y = blk(x, out_div=3.0, accum_join=join)
    assert events == [("block", DILATIONS[:2], None, 1.0), "join", ("unit", 2, addend, 3.0)]
    assert float(y[0, 0, 0]) == 3.0


def test_forward_resolves_a_join_that_waits_for_nothing_at_its_head(stub_block):
    """The first branch of the chain (k = 3) carries no addend: its join says so and the whole block fuses."""
    blk, events = stub_block
    x = torch.zeros(2, 32, 64)

    def join():
        events.append("join")
        return None

    join.pending = False
    with torch.no_grad():
        blk(x, accum_join=join)
    assert events == ["join", ("block", DILATIONS, None, 1.0)]


def test_forward_with_the_switch_off_runs_the_unit_loop(stub_block):
    blk, events = stub_block
    x = torch.zeros(2, 32, 64)
    blk.fuse_block = False
    with torch.no_grad():
        blk(x)
    assert [e[:2] for e in events] == [("unit", 0), ("unit", 1), ("unit", 2)]
    blk.fuse_block = True
    del events[:]
    for cv in blk.convs1:
        cv[1].split_exact = False  # the split switch: the predicate says no
    with torch.no_grad():
        blk(x)
    assert [e[:2] for e in events] == [("unit", 0), ("unit", 1), ("unit", 2)]


def test_a_causal_block_is_never_chained():
    """Its convolutions carry no split switch and have no resident-tile kernel: the block is not even asked."""
    from parallelwavegan_amd.layers import HiFiGANResidualBlock

    blk = HiFiGANResidualBlock(3, 32, DILATIONS, use_causal_conv=True)
    x = torch.zeros(2, 32, 64)
    assert blk._block_one_launch(x, 3, None, 1.0) == (0, x)
