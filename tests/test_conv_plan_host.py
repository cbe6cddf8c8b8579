"""CPU: what the conv forward's dispatcher decides (``ops.conv1d_plan``: csrc/conv1d.hip, conv_describe) for one layer of
every kind it tells apart, as a literal table, and the workspace query that goes with each answer.

The table was written out once by the build that preceded conv_describe (the plan entry then replayed the launcher's
cascade by hand) and is the record a later change of the dispatcher is held to: route family, tile, staging path, the
split factor of each of the three split rules of choose_cfg, tile order and grid.  Two rows are k = 63 filters: the 4 -> 4
one at dilation 1 still double-buffers on the 32 x 128 x 8 tile (141 KiB of LDS), the one at dilation 9 does not fit
160 KiB and falls back to the register-staged path.
"""
import ctypes

import pytest

from parallelwavegan_amd import _lib, ops
from tests import wgrad_cases

# (name, descriptor, concurrency hint, has_addends, plan)
ROWS = [
    ('mfma: generator layer, no split',
     dict(B=16, cin=128, cout=128, t_in=51200, t_out=51200, k=11, stride=1, dil=1, pad=5, groups=1), 1.0, False,
     {'family': 'mfma', 'tile_config': 11, 'ksplit': 1, 'dma': True, 'item_major': False, 'grid': (200, 2, 16)}),
    ('grouped: k = 41 stride 4, 4 -> 16 channels per group',
     dict(B=16, cin=64, cout=256, t_in=4096, t_out=1024, k=41, stride=4, dil=1, pad=20, groups=16), 1.0, False,
     {'family': 'grouped', 'tile_config': 0, 'ksplit': 0, 'dma': False, 'item_major': False, 'grid': (0, 0, 0)}),
    ('grouped layer with an addend: mfma',
     dict(B=16, cin=64, cout=256, t_in=4096, t_out=1024, k=41, stride=4, dil=1, pad=20, groups=16), 1.0, True,
     {'family': 'mfma', 'tile_config': 10, 'ksplit': 1, 'dma': True, 'item_major': False, 'grid': (8, 16, 16)}),
    ('single input channel',
     dict(B=2, cin=1, cout=16, t_in=2048, t_out=2048, k=15, stride=1, dil=1, pad=7, groups=1), 1.0, False,
     {'family': 'single_input_channel', 'tile_config': 0, 'ksplit': 0, 'dma': False, 'item_major': False, 'grid': (0, 0, 0)}),
    ('single input channel with an addend: mfma',
     dict(B=2, cin=1, cout=16, t_in=2048, t_out=2048, k=15, stride=1, dil=1, pad=7, groups=1), 1.0, True,
     {'family': 'mfma', 'tile_config': 10, 'ksplit': 1, 'dma': True, 'item_major': False, 'grid': (16, 1, 2)}),
    ('few output channels, LDS form',
     dict(B=1, cin=8, cout=2, t_in=4096, t_out=4096, k=9, stride=1, dil=1, pad=4, groups=1), 1.0, False,
     {'family': 'few_output_channels', 'tile_config': 0, 'ksplit': 0, 'dma': False, 'item_major': False, 'grid': (0, 0, 0)}),
    ('few output channels, stream form',
     dict(B=1, cin=8, cout=1, t_in=4096, t_out=4096, k=7, stride=1, dil=1, pad=3, groups=1), 1.0, False,
     {'family': 'few_output_channels', 'tile_config': 0, 'ksplit': 0, 'dma': False, 'item_major': False, 'grid': (0, 0, 0)}),
    ('k = 63, 4 -> 4: the double buffer of the 32 x 128 x 8 tile still fits (141 KiB)',
     dict(B=2, cin=4, cout=4, t_in=1024, t_out=1024, k=63, stride=1, dil=1, pad=31, groups=1), 1.0, False,
     {'family': 'mfma', 'tile_config': 10, 'ksplit': 1, 'dma': True, 'item_major': False, 'grid': (8, 1, 2)}),
    ('k = 63 dilation 9: double buffer above 160 KiB, register path',
     dict(B=2, cin=4, cout=4, t_in=1024, t_out=1024, k=63, stride=1, dil=9, pad=279, groups=1), 1.0, False,
     {'family': 'mfma', 'tile_config': 10, 'ksplit': 1, 'dma': False, 'item_major': False, 'grid': (8, 1, 2)}),
    ('reflect padding: register path',
     dict(B=2, cin=32, cout=64, t_in=1000, t_out=1000, k=7, stride=1, dil=1, pad=3, groups=1, pad_mode='reflect'), 1.0, False,
     {'family': 'mfma', 'tile_config': 10, 'ksplit': 1, 'dma': False, 'item_major': False, 'grid': (8, 2, 2)}),
    ('latency rule: S4 of tests/test_conv_cfg_matrix_gpu.py',
     dict(B=2, cin=72, cout=96, t_in=100, t_out=100, k=5, stride=1, dil=1, pad=2, groups=1), 1.0, False,
     {'family': 'mfma', 'tile_config': 13, 'ksplit': 2, 'dma': True, 'item_major': False, 'grid': (2, 2, 4)}),
    ('latency rule: 1024 -> 1 output layer',
     dict(B=16, cin=1024, cout=1, t_in=32, t_out=32, k=3, stride=1, dil=1, pad=1, groups=1), 1.0, False,
     {'family': 'mfma', 'tile_config': 10, 'ksplit': 8, 'dma': True, 'item_major': False, 'grid': (1, 1, 128)}),
    ('fill rule: 1024 -> 1024 k = 5 width 5',
     dict(B=16, cin=1024, cout=1024, t_in=21, t_out=21, k=5, stride=1, dil=1, pad=2, groups=1, width=5), 1.0, False,
     {'family': 'mfma', 'tile_config': 2, 'ksplit': 4, 'dma': True, 'item_major': False, 'grid': (1, 8, 64)}),
    ('fill rule under the concurrency hint 0.25',
     dict(B=16, cin=1024, cout=1024, t_in=21, t_out=21, k=5, stride=1, dil=1, pad=2, groups=1, width=5), 0.25, False,
     {'family': 'mfma', 'tile_config': 2, 'ksplit': 2, 'dma': True, 'item_major': False, 'grid': (1, 8, 32)}),
    ('underfill rule: single utterance',
     dict(B=1, cin=512, cout=512, t_in=800, t_out=800, k=7, stride=1, dil=1, pad=3, groups=1), 1.0, False,
     {'family': 'mfma', 'tile_config': 11, 'ksplit': 16, 'dma': True, 'item_major': False, 'grid': (4, 8, 16)}),
    ('underfill rule under the concurrency hint 0.25',
     dict(B=1, cin=512, cout=512, t_in=800, t_out=800, k=7, stride=1, dil=1, pad=3, groups=1), 0.25, False,
     {'family': 'mfma', 'tile_config': 11, 'ksplit': 4, 'dma': True, 'item_major': False, 'grid': (4, 8, 4)}),
    ('transposed, stride 8',
     dict(B=4, cin=512, cout=256, t_in=100, t_out=800, k=16, stride=8, dil=1, pad=4, groups=1, transposed=True), 1.0, False,
     {'family': 'mfma', 'tile_config': 9, 'ksplit': 4, 'dma': True, 'item_major': False, 'grid': (2, 16, 16)}),
]

# the environment switches that change a plan (the table is about the dispatcher without them)
OVERRIDES = ("PWG_TILE_ORDER", "PWG_ROWS32", "PWG_SPLIT_FILL", "PWG_SPLIT_UNDERFILL", "PWG_FORCE_CFG", "PWG_CONV_FILL_SCALE",
             "PWG_SMALL_CIN", "PWG_NO_GCONV")


def make_desc(row):
    s = dict(row[1])
    return ops.make_conv_desc(s.pop("B"), s.pop("cin"), s.pop("cout"), s.pop("t_in"), s.pop("t_out"), s.pop("k"),
                              s.pop("stride"), s.pop("dil"), s.pop("pad"), s.pop("groups"), **s)


@pytest.fixture(autouse=True)
def _no_overrides(monkeypatch):
    for name in OVERRIDES:  # (PWG_FORCE_CFG is read per call; the others must not have been set when the library loaded)
        monkeypatch.delenv(name, raising=False)


def test_the_table_covers_what_it_is_for():
    plans = [r[4] for r in ROWS]
    assert {p["family"] for p in plans} == set(ops.PLAN_FAMILIES)
    assert any(p["family"] == "mfma" and not p["dma"] and r[1].get("pad_mode") is None for r, p in zip(ROWS, plans))
    assert any(r[1].get("pad_mode") == "reflect" for r in ROWS) and any(r[1].get("transposed") for r in ROWS)
    assert sum(p["ksplit"] > 1 for p in plans) >= 3 and any(r[2] == 0.25 for r in ROWS) and any(r[3] for r in ROWS)


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_plan_and_workspace(row):
    _, s, hint, has_addends, want = row
    d = make_desc(row)
    with wgrad_cases.concurrency_hint(hint):
        plan = ops.conv1d_plan(d, has_addends=has_addends)
        ws = _lib.lib().pwg_conv1d_forward_workspace_floats(ctypes.byref(d))
    assert plan == want
    # the query is sized for the plan's slices: one y-shaped slab each, none for an unsplit launch
    assert ws == (plan["ksplit"] * s["B"] * s["cout"] * s["t_out"] * s.get("width", 1) if plan["ksplit"] > 1 else 0)
