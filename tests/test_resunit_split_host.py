"""CPU: what the split-operand residual unit's ``supported()`` declines (csrc/resunit_split.hip) and
the admission predicate of its routing (pure host logic)."""
from parallelwavegan_amd import _lib, ops
from parallelwavegan_amd.layers import conv as conv_mod
from parallelwavegan_amd.layers.conv import resunit_split_admitted


def _last_error():
    return _lib.lib().pwg_last_error().decode()


def test_supported_on_the_geometry_edges():
    for c in (32, 64):
        for k, d in ((3, 1), (3, 5), (7, 3), (11, 1), (11, 5)):
            for pair in (True, False):
                assert ops.resunit_split_supported(ops.make_resunit_desc(2, c, 100, k, d, pair)), (c, k, d, pair)
    assert not ops.resunit_split_supported(ops.make_resunit_desc(1, 128, 64, 3, 1))
    assert "channels = 128" in _last_error()
    assert not ops.resunit_split_supported(ops.make_resunit_desc(1, 32, 66, 3, 1))
    assert "multiple of 4" in _last_error()
    assert not ops.resunit_split_supported(ops.make_resunit_desc(1, 32, 64, 4, 1))
    assert "odd" in _last_error()
    assert not ops.resunit_split_supported(ops.make_resunit_desc(1, 32, 64, 3, 1, slope1=0.0))
    assert not ops.resunit_split_supported(ops.make_resunit_desc(0, 32, 64, 3, 1))
    # three planes of (H + (k - 1) d + up to 3) columns x (C + 8) bf16 within 80 KB: C = 64 takes a halo of 56 columns,
    # C = 32 one of 84
    assert ops.resunit_split_supported(ops.make_resunit_desc(1, 64, 64, 3, 28))
    assert not ops.resunit_split_supported(ops.make_resunit_desc(1, 64, 64, 3, 30))
    assert "LDS" in _last_error()
    assert ops.resunit_split_supported(ops.make_resunit_desc(1, 32, 64, 3, 40))
    assert not ops.resunit_split_supported(ops.make_resunit_desc(1, 32, 64, 3, 44))
    # a kernel so long that a tile keeps fewer than 64 outputs
    assert not ops.resunit_split_supported(ops.make_resunit_desc(1, 64, 64, 67, 1))


def test_admission_predicate(monkeypatch):
    monkeypatch.setattr(conv_mod, "RESUNIT_SPLIT_ADMITTED",
                        {(64, 7, True): ("pair", 30000), (32, 3, True): ("unit", 1000)})
    assert resunit_split_admitted(64, 7, True, 30000, False) == "pair"
    assert resunit_split_admitted(64, 7, True, 29999, False) is None, "short launches stay on the fp32 unit"
    assert resunit_split_admitted(64, 7, False, 1 << 20, False) is None, "a class that is not in the table"
    assert resunit_split_admitted(64, 7, True, 1 << 20, True) is None, "a gradient is needed"
    assert resunit_split_admitted(64, 7, True, 1 << 20, False, enabled=False) is None, "the switch is off"
    # no class under the column floor, whatever its row says
    assert conv_mod.RESUNIT_SPLIT_MIN_COLS == 20480
    assert resunit_split_admitted(32, 3, True, 20479, False) is None
    assert resunit_split_admitted(32, 3, True, 20480, False) == "unit"
    # admit_all: the one-launch unit, on every class
    assert resunit_split_admitted(32, 11, False, 1, False, admit_all=True) == "unit"
    assert resunit_split_admitted(64, 7, True, 1 << 20, False, admit_all=True) == "unit"
    assert resunit_split_admitted(32, 11, False, 1, True, admit_all=True) is None
    assert resunit_split_admitted(32, 11, False, 1, False, enabled=False, admit_all=True) is None


def test_admission_table_keeps_the_pinned_short_launches_on_the_fp32_unit():
    """tests/test_resunit_gpu.py pins the fp32 unit at 2 x 8192 columns under default settings."""
    assert conv_mod.RESUNIT_SPLIT_ADMITTED, "the table was filled from profiles/resunit_split.txt"
    for (c, k, pair), (form, min_cols) in conv_mod.RESUNIT_SPLIT_ADMITTED.items():
        assert c in (32, 64) and k % 2 == 1 and isinstance(pair, bool) and form in ("unit", "pair"), (c, k, pair, form)
        assert form == "unit" or pair, "the pair of split launches exists only for units of two convolutions"
        assert resunit_split_admitted(c, k, pair, 2 * 8192, False) is None
        assert resunit_split_admitted(c, k, pair, max(min_cols, 20480), False) == form


def test_block_routing_is_host_logic(monkeypatch):
    """The block asks the predicate with its own geometry: channels, kernel size, pair form, batch x T."""
    import torch

    from parallelwavegan_amd.layers import HiFiGANResidualBlock
    from parallelwavegan_amd.layers import residual_block as rb

    asked = []

    def spy(*a):
        asked.append(a)
        return None

    monkeypatch.setattr(rb, "resunit_split_admitted", spy)
    monkeypatch.setattr(rb.ops, "resunit_profitable", lambda d: False)  # no device here: the unit path ends
    blk = HiFiGANResidualBlock(7, 64, (1, 3))

    class FakeCuda(torch.Tensor):
        is_cuda = True

    x = torch.zeros(2, 64, 128).as_subclass(FakeCuda)
    with torch.no_grad():
        assert blk._unit_one_launch(0, x, None, 1.0) is None
    assert asked == [(64, 7, True, 256, False, blk.convs1[0][1].split_exact, False)]


def test_abi_version_is_unchanged():
    assert _lib.lib().pwg_abi_version() == 15 and _lib.ABI_VERSION == 15
