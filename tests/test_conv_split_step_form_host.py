"""CPU: which form of the reduction step the split-operand kernel's launch plan chooses (csrc/conv1d_split.hip,
``split_step_form``) -- pure host logic, answered by ``pwg_conv1d_split_step_form`` without a device --
and the additive ABI of the two entry points that came with it."""
import ctypes
import os
import re

import pytest

from parallelwavegan_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pwg_conv1d_split_step_form", "pwg_conv1d_split_forward_step")


def _res_conv(batch, ch, t, k, d=1):
    return ops.make_conv_desc(batch, ch, ch, t, t, k, dilation=d, pad_left=(k - 1) // 2 * d, pre_act="leaky_relu",
                              pre_slope=0.1)


@pytest.mark.parametrize("k", [7, 11])
@pytest.mark.parametrize("d", [1, 3, 5])
def test_plan_choice_for_the_forward_classes(k, d):
    """The admitted classes are the measured ones (every class the HiFi-GAN V1 forward sends to the
    kernel passed the keep rule): 256, 128 and 64 channels at 7 and 11 taps, at the benchmark length and at the
    single-utterance lengths alike -- the choice is by class, not by length."""
    for batch, frames in ((16, 800), (1, 800), (1, 100)):
        assert ops.conv1d_split_step_form(_res_conv(batch, 256, frames * 8, k, d)) == "streamed"
        assert ops.conv1d_split_step_form(_res_conv(batch, 128, frames * 64, k, d)) == "streamed"
        assert ops.conv1d_split_step_form(_res_conv(batch, 64, frames * 128, k, d)) == "streamed"


def test_classes_nobody_measured_stay_resident():
    """Streamed ONLY for the admitted classes: fewer than 7 taps or a single 32-channel chunk is resident."""
    for ch in (64, 128, 256):
        for k in (1, 3, 5):
            assert ops.conv1d_split_step_form(_res_conv(16, ch, 6400, k)) == "resident", (ch, k)
    for k in (7, 11):
        assert ops.conv1d_split_step_form(_res_conv(16, 32, 6400, k)) == "resident", k
        assert ops.conv1d_split_step_form(ops.make_conv_desc(16, 33, 32, 6400, 6400, k, pad_left=k // 2)) == "streamed", k
    assert ops.conv1d_split_step_form(ops.make_conv_desc(16, 80, 512, 800, 800, 7, pad_left=3)) == "streamed"


def test_unsupported_descriptors_and_bad_arguments_are_refused_with_a_message():
    lib = _lib.lib()
    grouped = ops.make_conv_desc(1, 32, 32, 64, 64, 7, pad_left=3, groups=2)
    assert lib.pwg_conv1d_split_step_form(ctypes.byref(grouped)) == 0
    assert b"conv1d_split" in lib.pwg_last_error()
    with pytest.raises(RuntimeError, match="groups"):
        ops.conv1d_split_step_form(grouped)
    transposed = ops.make_conv_desc(1, 128, 64, 64, 512, 16, stride=8, pad_left=4, transposed=True)
    assert lib.pwg_conv1d_split_step_form(ctypes.byref(transposed)) == 0
    ok = _res_conv(1, 32, 64, 7)
    # step_form outside 0 .. 2: refused before anything is dereferenced or launched
    for bad in (3, -1):
        rc = lib.pwg_conv1d_split_forward_step(ctypes.byref(ok), None, None, None, None, None, None, 16, 0, bad, None)
        assert rc != 0 and b"step_form" in lib.pwg_last_error(), bad
    rc = lib.pwg_conv1d_split_forward_step(ctypes.byref(ok), None, None, None, None, None, None, 16, 0, 2, None)
    assert rc != 0 and b"NULL" in lib.pwg_last_error()


def test_additive_abi():
    """Two new symbols, declared, exported and bound; no existing signature changed, so the ABI version stays 15."""
    assert _lib.ABI_VERSION == 15 == _lib.lib().pwg_abi_version()
    header = open(os.path.join(ROOT, "include", "pwg_kernels.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared"
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} is not bound"
    assert _lib.SIGNATURES["pwg_conv1d_split_forward_step"][1][:-2] == _lib.SIGNATURES["pwg_conv1d_split_forward_cfg"][1][:-1]
    assert "pwg_abi_version() stays 15" in header
