"""CPU: the weight-gradient configuration matrix of tests/wgrad_cases.py against ``ops.conv1d_wgrad_plan`` (host
arithmetic of csrc/conv1d_wgrad.hip, the decision functions the launcher itself calls): every case still reaches the
variant it is there for, the table as a whole covers every variant the dispatcher can select, and the two workspace
queries -- separate code -- ask for what the plan says the launch needs."""
import ctypes

import pytest

from parallelwavegan_amd import _lib, ops
from tests import wgrad_cases as W


def _skip_under_overrides():
    names = W.overrides_set()
    if names:
        pytest.skip(f"{', '.join(names)} set: the plan is no longer the dispatcher's own")


@pytest.mark.parametrize("case", W.CASES, ids=[c["name"] for c in W.CASES])
def test_case_reaches_its_variant(case):
    _skip_under_overrides()
    plan = W.plan_of(case)
    missed = {k: (v, plan.get(k)) for k, v in case["expect"].items() if plan.get(k) != v}
    assert not missed, (f"case {case['name']} no longer exercises "
                        + ", ".join(f"{k}={want!r} (the plan says {got!r})" for k, (want, got) in missed.items())
                        + f"; full plan: {plan}")


def test_table_covers_every_variant():
    _skip_under_overrides()
    covered = set()
    for case in W.CASES:
        covered |= W.covered(case, W.plan_of(case))
    missing = W.REQUIRED - covered
    assert not missing, f"no case of tests/wgrad_cases.py exercises {sorted(missing, key=str)}"


@pytest.mark.parametrize("case", W.CASES, ids=[c["name"] for c in W.CASES])
def test_workspace_queries_agree_with_the_plan(case):
    desc = W.make_desc(case)
    lib = _lib.lib()
    with W.concurrency_hint(case["hint"]):
        plain = lib.pwg_conv1d_backward_weight_workspace_floats(ctypes.byref(desc))
        wn = lib.pwg_conv1d_backward_weight_wn_workspace_floats(ctypes.byref(desc))
    assert plain == W.plan_of(case, weight_norm=False)["workspace_floats"]
    assert wn == W.plan_of(case, weight_norm=True)["workspace_floats"]


@pytest.mark.parametrize("case", W.CASES, ids=[c["name"] for c in W.CASES])
def test_workspace_without_a_bias_row(case):
    """has_bias=False: the plain entry point's slabs lose the bias row (dW only), a single slice needs none; the
    weight-norm entry point asks for its query's size whatever the bias."""
    plan = W.plan_of(case, weight_norm=False, has_bias=False)
    if plan["path"] == "gconv":
        assert plan["workspace_floats"] == W.plan_of(case, weight_norm=False)["workspace_floats"]
    else:
        g = case["groups"]
        w_elems = case["cout"] * case["cin"] // g * case["k"]
        # (only the MFMA kernel stores a single slice's gradients itself; the other kernels always write slabs)
        direct = plan["path"] == "mfma" and plan["finisher"] == "direct"
        assert plan["workspace_floats"] == (0 if direct else plan["slabs"] * w_elems)
    if case["wn"]:
        assert (W.plan_of(case, weight_norm=True, has_bias=False)["workspace_floats"]
                == W.plan_of(case, weight_norm=True)["workspace_floats"])


def test_plan_follows_the_concurrency_hint():
    """The launcher reads the hint, so the query must: fewer resident workgroups, fewer slices."""
    _skip_under_overrides()
    case = W.BY_NAME["hint_below_1"]
    alone = ops.conv1d_wgrad_plan(W.make_desc(case))
    shared = W.plan_of(case)
    assert shared["splits"] < alone["splits"], (shared, alone)
    assert ops.conv1d_wgrad_plan(W.make_desc(case)) == alone  # (the hint was restored)


def test_plan_refuses_what_the_launcher_refuses():
    """The launcher's own checks, in the launcher's words (one shared function each)."""
    def refused(match, *a, weight_norm=False, **k):
        with pytest.raises(RuntimeError, match=match):
            ops.conv1d_wgrad_plan(ops.make_conv_desc(*a, **k), weight_norm=weight_norm)

    # a weight-normalised row longer than the fused finisher's LDS row buffer (functional.conv_param_grads routes it
    # to the two-kernel finish); the same layer without weight norm is fine
    refused("exceeds the LDS row buffer", 2, 16384, 8, 4, 4, 1, weight_norm=True)
    assert ops.conv1d_wgrad_plan(ops.make_conv_desc(2, 16384, 8, 4, 4, 1))["path"] == "mfma"
    refused("bad groups", 1, 6, 8, 16, 16, 3, groups=4)
    refused("only zero padding", 2, 8, 8, 16, 16, 3, pad_left=1, pad_mode="reflect")
    refused("above 4 GiB", 64, 512, 512, 40000, 40000, 3, pad_left=1)
    # a slope outside [0, 1] on every path that applies max(v, slope * v): mfma, single input channel, 1 x 1
    refused("slope 1.5 outside", 2, 40, 40, 64, 64, 3, pad_left=1, pre_act="leaky_relu", pre_slope=1.5)
    refused("slope 1.5 outside", 2, 1, 16, 2100, 2100, 15, pad_left=7, pre_act="leaky_relu", pre_slope=1.5)
    refused("slope 1.5 outside", 8, 48, 48, 4096, 4096, 1, pre_act="leaky_relu", pre_slope=1.5)
    refused("dilation with stride", 2, 40, 40, 16, 37, 4, stride=2, dilation=2, transposed=True)
    refused("of LDS", 2, 128, 128, 4000, 100, 41, stride=13, dilation=300)
