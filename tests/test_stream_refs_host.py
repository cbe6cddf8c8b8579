"""CPU: the references of tests/stream_refs.py are themselves checked -- composed chunk by chunk over a partition of a
signal they equal one whole-signal float64 evaluation by torch's own convolutions -- and the table of
tests/test_conv_stream_matrix_gpu.py is checked without a GPU: the float32 room under its bar, the sensitivity of
every case to a missing channel, tap or history column, the tile each case claims (``pwg_conv1d_stream_plan``), and
the completeness of its ``COVERED`` map over the entry points of csrc/conv1d_stream.hip."""
import importlib
import os
import re

import pytest
import torch
import torch.nn.functional as F

from parallelwavegan_amd import ops
from tests import stream_refs as R
from tests import test_conv_stream_matrix_gpu as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = torch.float64
TIGHT = 1e-12  # two float64 evaluations of O(1) quantities over at most a few hundred terms (test_wavenet_refs_host.py)
PAD_OF = {"zero": "constant", "replicate": "replicate", "reflect": "reflect"}
EPI = dict(out_mul=0.75, out_div=3.0, post_act="leaky_relu", post_slope=0.2)


def _close(a, b, tol=TIGHT):
    assert a.shape == b.shape, (a.shape, b.shape)
    err = (a - b).abs().max().item()
    assert err <= tol * max(1.0, b.abs().max().item()), err


def _rand(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s: torch.randn(*s, dtype=D, generator=g)


def _split(t, pieces, r=1):
    out, at = [], 0
    for n in pieces:
        out.append(t[..., at * r:(at + n) * r])
        at += n
    assert at * r == t.shape[-1]
    return out


# ------------------------------------------------------------------------------------------------ composition
# (k, d, partitions of T = 40): H = 0, 1, 12 and 27, with pieces shorter than H; a reflect-padded stream starts with
# H + 1 columns
LAYERS = [(1, 1), (2, 1), (5, 3), (4, 9)]
T = 40


def _partitions(first):
    return [(T,), (first,) + (1,) * (T - first), (first, 2, 1, 5, T - first - 8)]


@pytest.mark.parametrize("pad", ["zero", "replicate", "reflect"])
@pytest.mark.parametrize("k,d", LAYERS)
@pytest.mark.parametrize("pre", [None, "leaky_relu", "relu"])
def test_chunks_compose_to_the_padded_convolution(pad, k, d, pre):
    r = _rand(100 * k + d)
    H = (k - 1) * d
    x, w, b, add1, add2 = r(2, 6, T), r(5, 6, k), r(5), r(2, 5, T), r(2, 5, T)
    whole = F.conv1d(F.pad(R.act(x, pre, 0.1), (H, 0), mode=PAD_OF[pad]), w, dilation=d)
    whole = R.epilogue(whole, b, add1, add2, **EPI)
    for pieces in _partitions(H + 1 if pad == "reflect" else 1):
        hist, outs = None, []
        for xn, a1, a2 in zip(_split(x, pieces), _split(add1, pieces), _split(add2, pieces)):
            win = R.window(hist, xn, H, pad)
            outs.append(R.conv_chunk(win, w, d, pre, 0.1, bias=b, add1=a1, add2=a2, **EPI))
            hist = R.history(hist, xn, H, pad == "replicate")
            assert hist.shape[-1] == H
        _close(torch.cat(outs, -1), whole)
        # the history after the last chunk is the padded signal's tail, raw
        assert torch.equal(hist, F.pad(x, (H, 0), mode=PAD_OF[pad])[..., T:])


@pytest.mark.parametrize("pad", ["zero", "replicate"])
@pytest.mark.parametrize("s", [2, 4, 8])
def test_chunks_compose_to_the_cropped_transposed_convolution(pad, s):
    r = _rand(s)
    x, w, b, add1 = r(2, 6, T), r(6, 5, 2 * s), r(5), r(2, 5, T * s)
    xa = F.pad(R.act(x, "leaky_relu", 0.1), (1, 0), mode=PAD_OF[pad])
    whole = R.epilogue(F.conv_transpose1d(xa, w, None, stride=s)[:, :, s:-s], b, add1, **EPI)
    for pieces in _partitions(1):
        hist, outs = None, []
        for xn, a1 in zip(_split(x, pieces), _split(add1, pieces, s)):
            win = R.window(hist, xn, 1, pad, transposed=True)
            outs.append(R.transposed_chunk(win, w, s, "leaky_relu", 0.1, bias=b, add1=a1, **EPI))
            hist = R.history(hist, xn, 1, pad == "replicate")
        _close(torch.cat(outs, -1), whole)


@pytest.mark.parametrize("s", [0, 4])
@pytest.mark.parametrize("delays", [(0, 3), (7, 50), (50, 1)])
def test_delayed_chunks_compose_to_the_host_delayed_signal(s, delays):
    """A layer whose output is ``out_delay`` columns late, with addends that arrive ``delay_i`` columns early, pushed
    ``frames`` at a time past the utterance's end: the chunks' delay lines and windows (the window rule, from the frames
    before and left) give the whole signal with host-delayed addends, zero outside [out_delay, out_delay + F * rate)."""
    r = _rand(17 + s + delays[0])
    rate, k, d = (s, 2 * s, 1) if s else (1, 3, 2)
    H = 1 if s else (k - 1) * d
    frames, pushes, out_delay = 23, (1, 2, 9, 4, 1, 6, 12, 5), 11
    total = sum(pushes)
    assert total * rate > out_delay + frames * rate  # the stream is flushed past the end of the utterance
    x, b = r(2, 6, total), r(5)
    w = r(6, 5, k) if s else r(5, 6, k)
    adds = [r(2, 5, total * rate) for _ in delays]
    if s:
        acc = F.conv_transpose1d(F.pad(x, (1, 0)), w, None, stride=s)[:, :, s:-s]
    else:
        acc = F.conv1d(F.pad(x, (H, 0)), w, dilation=d)
    late = [F.pad(a, (dl, 0))[..., :total * rate] for a, dl in zip(adds, delays)]
    whole = R.zero_outside(R.epilogue(acc, b, late[0], late[1], **EPI), out_delay, out_delay + frames * rate)
    hist, line, outs, before = None, [None, None], [], 0
    for n in pushes:
        xn = x[..., before:before + n]
        an = [a[..., before * rate:(before + n) * rate] for a in adds]
        valid = R.slot_window(out_delay, rate, n * rate, before, frames - before, True)
        win = R.window(hist, xn, H, "zero", bool(s))
        acc_n = R.contract_transposed(win, w, s) if s else R.contract(win, w, d)
        outs.append(R.delayed_chunk(acc_n, valid, an[0], line[0], delays[0], an[1], line[1], delays[1], bias=b, **EPI))
        hist = R.history(hist, xn, H)
        line = [R.line_out(line[i], an[i], delays[i]) for i in range(2)]
        before += n
    _close(torch.cat(outs, -1), whole)


def test_window_rule():
    assert R.slot_window(7, 1, 12, 0, 9, True) == (7, 12)
    assert R.slot_window(7, 1, 12, 5, 2, True) == (2, 9)
    assert R.slot_window(10, 4, 48, 5, 2, True) == (0, 18)
    assert R.slot_window(10, 4, 48, 1, 0, False) == (6, 48)       # the utterance's length is not known yet
    assert R.slot_window(10, 4, 48, 0, -9, True) == (10, 0)        # past its end: empty
    assert R.slot_window(100, 1, 12, 0, 50, True) == (12, 12)      # the delay is longer than the push
    assert R.slot_window(3, 2, 8, 2 ** 30, 2 ** 30, True) == (0, 8)  # 64-bit positions


@pytest.mark.parametrize("k,d", [(7, 1), (3, 27), (3, 1)])
def test_mirrored_chunks_compose_to_the_reflect_padded_convolution(k, d):
    """The non-causal reflect-padded layer in causal form on an axis shifted by p = (k - 1) d / 2: stream output column
    q is whole column q - p; the stream is the utterance followed by stored zeros."""
    r = _rand(k * d)
    H = (k - 1) * d
    p, T_ = H // 2, H + 9
    x, w, b = r(2, 6, T_), r(5, 6, k), r(5)
    whole = R.epilogue(F.conv1d(F.pad(x, (p, p), mode="reflect"), w, dilation=d), b, post_act="tanh")
    stream = F.pad(x, (0, p + 3))
    for pieces in [(T_ + p + 3,), (1,) * (T_ + p + 3), (3, 1, T_ - 6, 2, p + 3)]:
        hist, outs, at = None, [], 0
        for xn in _split(stream, pieces):
            n = xn.shape[-1]
            in_lo, in_hi = -at, T_ - at
            win = R.mirror_window(hist, xn, H, in_lo, in_hi)
            outs.append(R.zero_outside(R.conv_chunk(win, w, d, bias=b, post_act="tanh"), in_lo + p, in_hi + p))
            hist = R.history(hist, xn, H)
            at += n
        y = torch.cat(outs, -1)
        _close(y[..., p:p + T_], whole)
        assert y[..., :p].abs().max() == 0 and y[..., p + T_:].abs().max() == 0
    assert [R.mirror_column(t, -2, 5) for t in (-4, -3, -2, 4, 5, 6)] == [0, -1, -2, 4, 3, 2]
    assert R.mirror_column(10 ** 6, -2, None) == 10 ** 6


# ------------------------------------------------------------------------------------------------ the GPU table
ROWS = [(c, n) for c in M.EVERY_CASE for n in c.ns]
ROW_IDS = [f"{c.id}-n{n}" for c, n in ROWS]


@pytest.fixture(scope="module")
def room():
    worst = {}
    yield worst
    if worst:
        k = max(worst, key=worst.get)
        print(f"float32 vs float64, worst rel-to-max error {worst[k]:.3e} ({worst[k] / M.RTOL:.2%} of RTOL) at {k}")


@pytest.mark.parametrize("c,n", ROWS, ids=ROW_IDS)
def test_room_under_the_bar(c, n, room):
    """The float32 CPU evaluation of the same formulas on the same data stays well inside the GPU bar: what the kernel
    is allowed beyond it is accumulation order, not the data's conditioning.  (Measured: the worst row, tr-16-8-24 n = 9, is 1.1e-6 from float64,
    3.7 % of RTOL; the assertion allows 10 %.)"""
    t = M.inputs(c, n)
    want, got = M.reference(c, t), M.reference(c, t, torch.float32).double()
    err = (got - want).abs().max().item() / want.abs().max().item()
    room[f"{c.id}-n{n}"] = err
    assert err <= 0.1 * M.RTOL, err


@pytest.mark.parametrize("c,n", ROWS, ids=ROW_IDS)
def test_sensitivity(c, n):
    """Zeroing the last real input channel, the last tap of the reduction or the oldest history column moves the float64
    result by at least 100 x RTOL of its largest magnitude: a bound relative to the maximum cannot hide a missing channel
    group, tap or column."""
    t = M.inputs(c, n)
    want = M.reference(c, t)
    floor = 100 * M.RTOL * want.abs().max().item()
    moved = lambda other: (M.reference(c, other[0], w=other[1]) - want).abs().max().item()  # noqa: E731
    x, hist, w = t.x.clone(), None if t.hist is None else t.hist.clone(), t.w.clone()
    x[:, -1] = 0
    if hist is not None:
        hist[:, -1] = 0
    assert moved((t._replace(x=x, hist=hist), None)) >= floor, "last input channel"
    if c.s:
        w[:, :, :c.s] = 0   # tap 1 of the two: x[j] with w[phase]
    else:
        w[:, :, -1] = 0
    assert moved((t, w)) >= floor, "last tap"
    if t.hist is not None:
        hist = t.hist.clone()
        hist[..., 0] = 0
        assert moved((t._replace(hist=hist), None)) >= floor, "oldest history column"


def _claims():
    for c in M.EVERY_CASE:
        rows = 32 if c in M.TILE_CASES else 16
        for n, cols in zip(c.ns, c.tiles):
            yield c, n, (rows, cols)


def test_tiles_are_what_the_cases_claim():
    seen = set()
    for c, n, tile in _claims():
        plan = ops.conv1d_stream_plan(M.desc_of(c, n))
        m = c.cout * M.rate(c)
        assert plan["tile"] == tile, (c.id, n, plan)
        assert plan["grid"] == (-(-n // tile[1]), -(-m // tile[0]), c.B), (c.id, n, plan)
        seen.add(plan["tile"])
    assert seen == {(16, 16), (16, 32), (16, 64), (32, 64)}, seen
    for c in M.TILE_CASES:  # one item fewer: below the threshold of 2 x 256 workgroups
        assert ops.conv1d_stream_plan(M.desc_of(c, c.ns[0], B=31))["tile"] == (16, 64)


def test_table_covers_its_axes():
    rows = M.CASES
    assert 30 <= len(rows) <= 40
    plain = [c for c in rows if not c.s]
    assert {c.cin for c in rows} >= {1, 48, 64, 72, 130, 512}
    assert {c.k for c in plain} >= {1, 2, 3, 4, 5, 7, 8, 9, 11}
    assert all(c.cin >= 128 for c in plain if c.k == 11)
    assert {M.hist_cols(c) for c in plain} >= {0, 1, 144} and sum(M.hist_cols(c) == 144 for c in plain) >= 2
    assert any(min(c.ns) < M.hist_cols(c) < max(c.ns) for c in plain)
    assert {n for c in rows for n in c.ns} >= {1, 15, 16, 17, 32, 33, 64, 65, 130}
    assert {c.cout for c in plain} >= {1, 24, 40, 128, 136}
    assert {(c.k, c.s, c.cout, c.start) for c in rows if c.s} >= {(k, s, co, st) for k, s, co in
                                                                  [(4, 2, 1), (8, 4, 24), (8, 4, 40), (16, 8, 24)]
                                                                  for st in (False, True)}
    assert {(c.pad, c.start) for c in rows} >= {("zero", True), ("replicate", True), ("reflect", True)}
    assert {c.pre for c in rows} == {None, "leaky_relu", "relu"} and {c.post for c in rows} == {None, "tanh", "leaky_relu"}
    alone = [(c.bias, c.add1, c.add2, c.mul != 1.0, c.div != 1.0, c.post is not None) for c in rows]
    for i in range(6):
        assert tuple(j == i for j in range(6)) in alone, f"epilogue term {i} never runs alone"
    assert (True,) * 6 in alone
    for c in rows:
        if c.pad == "reflect" and c.start:
            assert c.ns[0] == M.hist_cols(c) + 1


def test_history_above_the_cap_is_refused():
    d = ops.make_conv_desc(1, 16, 16, 8, 8, 2, 1, 145, 145, 1)
    assert not ops.conv1d_stream_supported(d)
    with pytest.raises(RuntimeError, match="history of 145 columns"):
        ops.conv1d_stream_plan(d)
    assert ops.conv1d_stream_plan(ops.make_conv_desc(1, 16, 16, 8, 8, 2, 1, 144, 144, 1))["tile"] == (16, 16)


# ------------------------------------------------------------------------------------------------ completeness
def _entry_points():
    src = open(os.path.join(ROOT, "parallelwavegan_amd", "csrc", "conv1d_stream.hip")).read()
    return re.findall(r'^extern "C" (?:int|size_t) (pwg_\w+)\(', src, re.M)


def test_every_entry_point_names_the_test_that_drives_it():
    names = _entry_points()
    assert len(names) == 9 and "pwg_conv1d_stream_forward" in names and "pwg_conv1d_stream_plan" in names, names
    assert len(re.findall(r'extern "C"', open(os.path.join(ROOT, "parallelwavegan_amd", "csrc", "conv1d_stream.hip")).read())) \
        == len(names), "an extern \"C\" definition the pattern above does not see"
    gpu = importlib.import_module("tests.test_conv_stream_matrix_gpu")
    missing = [n for n in names if n not in gpu.COVERED]
    assert not missing, f"entry points with no direct test: {missing}"
    stale = [n for n in gpu.COVERED if n not in names]
    assert not stale, f"COVERED names entry points that no longer exist: {stale}"
    marks = getattr(gpu, "pytestmark", [])
    marks = list(marks) if isinstance(marks, (list, tuple)) else [marks]
    for name, where in gpu.COVERED.items():
        fn = getattr(gpu, where, None)
        assert callable(fn) and where.startswith("test_"), f"{name}: no test function {where}"
        assert any(m.name == "gpu" for m in marks + list(getattr(fn, "pytestmark", []))), f"{where} is not marked gpu"
