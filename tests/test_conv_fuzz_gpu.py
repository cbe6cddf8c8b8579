"""GPU: seeded random sweep of the conv1d family (forward, data gradient, weight / bias gradient; plain,
strided, dilated, grouped and transposed; ragged lengths down to a single output column) against torch
CPU fp32 -- tools/fuzz_conv.py run for a fixed seed; and its second sweep over the fused epilogue terms, pad
modes, causal padding and misaligned views against float64."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu


def _fuzz_conv():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import fuzz_conv

    return fuzz_conv


def test_random_conv_configurations(device):
    fuzz_conv = _fuzz_conv()

    bad = fuzz_conv.run(120, 7)
    assert not bad, bad[:5]


def test_random_epilogue_configurations(device):
    """80 cases of ``fuzz_conv.run_epilogue`` at seed 11 (78 pass the generator's geometry filters and reach the
    planner); a case is skipped only by those filters or by a library answer of "unsupported"."""
    from tests.util import poison_empty, poison_lds

    with poison_lds(), poison_empty():
        bad, ran = _fuzz_conv().run_epilogue(80, 11)
    assert not bad, bad[:5]
    assert ran >= 0.85 * 80, ran
