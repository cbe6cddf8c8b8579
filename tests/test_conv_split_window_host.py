"""CPU: which form of the window staging the split-operand kernel's launch plan chooses (csrc/conv1d_split.hip,
``split_window_form``; DESIGN.md s9.1, "The prefetched window") -- pure host logic, answered by
``pwg_conv1d_split_window_form`` without a device --, the additive ABI of the two entry points that came with it, and the
admission predicate of the few-tap classes (``layers/conv.py``, ``split_fewtap_admitted``)."""
import ctypes
import os
import re

import pytest

from parallelwavegan_amd import _lib, ops
from parallelwavegan_amd.layers import conv as conv_mod
from parallelwavegan_amd.layers.conv import split_admitted, split_fewtap_admitted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pwg_conv1d_split_window_form", "pwg_conv1d_split_forward_window")


def _res_conv(batch, ch, t, k, d=1):
    return ops.make_conv_desc(batch, ch, ch, t, t, k, dilation=d, pad_left=(k - 1) // 2 * d, pre_act="leaky_relu",
                              pre_slope=0.1)


@pytest.mark.parametrize("k", [3, 7, 11])
@pytest.mark.parametrize("d", [1, 3, 5])
def test_plan_choice_for_the_forward_classes(k, d):
    """No class passed the keep rule (profiles/split_window.txt: at 16 x 800 frames the prefetched window is disjointly
    slower on every class measured), so the plan answers staged for every class the HiFi-GAN V1 forward sends to the
    kernel, at every length."""
    for batch, frames in ((16, 800), (1, 800), (1, 100)):
        assert ops.conv1d_split_window_form(_res_conv(batch, 256, frames * 8, k, d)) == "staged"
        assert ops.conv1d_split_window_form(_res_conv(batch, 128, frames * 64, k, d)) == "staged"
        assert ops.conv1d_split_window_form(_res_conv(batch, 64, frames * 128, k, d)) == "staged"


def test_what_the_prefetched_form_does_not_cover_is_staged_or_refused():
    lib = _lib.lib()
    # no 16-B staging: a row length that is no multiple of 4
    assert ops.conv1d_split_window_form(_res_conv(2, 64, 402, 3, 5)) == "staged"
    # planes and raw regions that would not leave three workgroups to a CU: 128 + 54 columns, 45 KB + 24 KB
    assert ops.conv1d_split_window_form(_res_conv(16, 128, 6400, 3, 27)) == "staged"
    grouped = ops.make_conv_desc(1, 32, 32, 64, 64, 3, pad_left=1, groups=2)
    assert lib.pwg_conv1d_split_window_form(ctypes.byref(grouped)) == 0
    assert b"conv1d_split" in lib.pwg_last_error()
    with pytest.raises(RuntimeError, match="groups"):
        ops.conv1d_split_window_form(grouped)
    transposed = ops.make_conv_desc(1, 128, 64, 64, 512, 16, stride=8, pad_left=4, transposed=True)
    assert lib.pwg_conv1d_split_window_form(ctypes.byref(transposed)) == 0
    assert b"transposed" in lib.pwg_last_error()


def test_bad_arguments_are_refused_before_any_pointer_is_read():
    lib = _lib.lib()
    ok = _res_conv(1, 64, 64, 3)
    null = (ctypes.byref(ok), None, None, None, None, None, None)
    # window_form outside 0 .. 2: refused before anything is dereferenced or launched
    for bad in (3, -1):
        assert lib.pwg_conv1d_split_forward_window(*null, 16, 0, 0, bad, None) != 0
        assert b"window_form" in lib.pwg_last_error(), bad
    assert lib.pwg_conv1d_split_forward_window(*null, 16, 0, 3, 0, None) != 0
    assert b"step_form" in lib.pwg_last_error()
    for form in (0, 1, 2):
        assert lib.pwg_conv1d_split_forward_window(*null, 16, 0, 0, form, None) != 0
        assert b"NULL" in lib.pwg_last_error(), form
    # a forced 2 on a launch the form does not cover is refused with a message (the pointers are never read: the
    # buffer is a few bytes, the launch would be 2 x 64 x 402 floats)
    buf = (ctypes.c_char * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)  # 16-B aligned, as a weight image must be
    odd = _res_conv(2, 64, 402, 3, 5)
    args = (ctypes.byref(odd), p, p, None, None, None, p)
    assert lib.pwg_conv1d_split_forward_window(*args, 16, 0, 0, 2, None) != 0
    assert b"16-B staging" in lib.pwg_last_error()
    even = _res_conv(2, 64, 404, 3, 5)
    args = (ctypes.byref(even), p, p, None, None, None, p)
    assert lib.pwg_conv1d_split_forward_window(*args, 16, 0, 2, 2, None) != 0
    assert b"streamed" in lib.pwg_last_error()


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
    assert (_lib.SIGNATURES["pwg_conv1d_split_forward_window"][1][:-2]
            == _lib.SIGNATURES["pwg_conv1d_split_forward_step"][1][:-1])
    # the step form keeps its answers: the window form is a second axis, not a third step form
    for k in (1, 3, 5):
        assert ops.conv1d_split_step_form(_res_conv(16, 128, 6400, k)) == "resident"
    assert ops.conv1d_split_step_form(_res_conv(16, 128, 6400, 7)) == "streamed"
    assert sorted(ops.STEP_FORMS.values()) == ["resident", "streamed"]


def test_fewtap_admission_predicate(monkeypatch):
    monkeypatch.setattr(conv_mod, "SPLIT_FEWTAP_ADMITTED", {(128, 128, 3): 6400, (48, 48, 3): 100})
    assert split_fewtap_admitted(128, 128, 3, 6400, False)
    assert not split_fewtap_admitted(128, 128, 3, 6399, False)  # the class's floor
    assert split_fewtap_admitted(48, 48, 3, 6400, False)
    assert not split_fewtap_admitted(48, 48, 3, 6399, False)  # never under SPLIT_FEWTAP_MIN_COLS
    assert not split_fewtap_admitted(128, 128, 3, 1 << 20, True)  # a gradient is needed
    assert not split_fewtap_admitted(128, 128, 3, 1 << 20, False, enabled=False)  # the switch is off
    assert not split_fewtap_admitted(256, 256, 3, 1 << 20, False)  # not listed
    assert not split_fewtap_admitted(128, 128, 5, 1 << 20, False)
    assert split_fewtap_admitted(256, 256, 3, 4, False, admit_all=True)
    assert not split_fewtap_admitted(256, 256, 3, 4, True, admit_all=True)
    assert not split_fewtap_admitted(256, 256, 3, 4, False, enabled=False, admit_all=True)


def test_default_tables():
    assert conv_mod.SPLIT_FEWTAP_MIN_COLS >= 6400
    for (c_in, c_out, k), cols in conv_mod.SPLIT_FEWTAP_ADMITTED.items():
        assert k < 7 and cols >= 6400, (c_in, c_out, k, cols)
    for (ch, k, _), (_, cols) in conv_mod.RESUNIT_SPLIT_ADMITTED.items():
        if ch == 32 and k == 3:
            assert cols > 25600, cols
    # the k >= 7 table and its predicate are what they were
    assert all(k >= 7 for _, _, k in conv_mod.SPLIT_ADMITTED)
    for ch in (128, 256):
        assert not split_admitted(ch, ch, 3, 1 << 20, False)
        assert split_admitted(ch, ch, 7, 6400, False)


def test_the_route_consults_both_tables(monkeypatch):
    from parallelwavegan_amd.layers.conv import Conv1d

    cv = Conv1d(128, 128, 3, padding=1)
    desc = cv.make_desc(16, 51200)
    monkeypatch.setattr(conv_mod, "SPLIT_FEWTAP_ADMITTED", {})
    assert not cv._split_route(desc)
    monkeypatch.setattr(conv_mod, "SPLIT_FEWTAP_ADMITTED", {(128, 128, 3): 6400})
    assert cv._split_route(desc)
    assert not cv._split_route(desc, needs_grad=True)
    assert not cv._split_route(cv.make_desc(1, 6396))
    monkeypatch.setattr(type(cv), "split_exact", False)
    assert not cv._split_route(desc)
