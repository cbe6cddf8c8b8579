"""GPU: the element-wise, norm and reduction kernels of csrc/elementwise.hip and csrc/reduce_optim.hip one by one against
the float64 references of tests/elementwise_refs.py, at the smallest shapes that still reach each edge (the window cut by
the padding, the tie, the row that is no multiple of the workgroup, the second trip of the grid-stride loop).

Every case runs under ``poison_empty`` (an output element nobody wrote is NaN) and twice (``torch.equal``: every kernel
here claims a fixed summation order).  Three kinds of comparison, none of them measured on the kernels:

* ``bits``: copies, selections and single correctly-rounded operations equal the reference rounded to float32;
* ``("sum", n)``: ``|err| <= (n + 4) * 2^-24 * S`` with ``S`` the sum of the absolute values of the element's terms --
  the forward-error bound of a sum of ``n`` rounded terms in ANY order; the 4 covers the roundings that are not
  additions (a product, a scale, a division by the window length: correctly rounded or not, at most 2.5 ulp);
* ``meas``: results that pass through ``tanhf``, ``expf``, ``logf``, ``sqrtf``, ``rsqrtf`` or a division get 4 times
  the largest error of torch's float32 CPU evaluation of the same formula plus 4 ulp of the element's magnitude.

Each comparison prints ``<operation>: err/bound`` (the largest ratio over the elements), the slack that was used.
"""
import itertools
import math

import numpy as np
import pytest
import torch

from parallelwavegan_amd import _lib, functional as Fn, ops
from parallelwavegan_amd.ops import _ptr, _stream
from parallelwavegan_amd.utils import streaming
from tests import elementwise_refs as R
from tests.util import poison_empty

D = torch.float64
SLOPE = R.f32(0.2)
EPS_NORM = R.f32(1e-5)

# entry point -> the test below that drives it directly, or the existing test file that does
COVERED = {
    "pwg_act_backward": "test_act_backward",
    "pwg_weight_norm_backward": "test_weight_norm",
    "pwg_avg_pool1d_forward": "test_avg_pool",
    "pwg_avg_pool1d_backward": "test_avg_pool",
    "pwg_pad1d_forward": "test_pad",
    "pwg_pad1d_backward": "test_pad",
    "pwg_frame_fold_forward": "test_frame_fold",
    "pwg_frame_fold_backward": "test_frame_fold",
    "pwg_stft_mag_forward": "test_stft_mag",
    "pwg_stft_mag_backward": "test_stft_mag",
    "pwg_log_clamp_forward": "test_log_clamp",
    "pwg_log_clamp_backward": "test_log_clamp",
    "pwg_spectral_norm_forward": "tests/test_discriminator_gpu.py",
    "pwg_spectral_norm_forward_saved": "test_spectral_norm",
    "pwg_spectral_norm_backward": "test_spectral_norm",
    "pwg_gate_forward": "test_gates",
    "pwg_gate_backward": "test_gates",
    "pwg_stretch_conv_forward": "test_stretch_conv",
    "pwg_stretch_conv_backward": "test_stretch_conv",
    "pwg_stretch_conv_stream": "tests/test_stream_pwg_gpu.py",
    "pwg_stretch_conv_stream_delayed": "tests/test_stream_pwg_lookahead_gpu.py",
    "pwg_delay_line_forward": "tests/test_stream_pwg_lookahead_gpu.py",
    "pwg_add3_div": "test_add3_div",
    "pwg_wave_to_pcm16": "test_wave_to_pcm16",
    "pwg_normalize_transpose": "test_normalize_transpose",
    "pwg_zero_tail": "tests/test_ragged_gpu.py",
    "pwg_mirror_tail": "tests/test_ragged_melgan_gpu.py",
    "pwg_gather_crop": "tests/test_device_collater_gpu.py",
    "pwg_instance_norm_forward": "test_instance_norm",
    "pwg_instance_norm_backward": "test_instance_norm",
    "pwg_upsample_nearest_forward": "test_upsample_nearest",
    "pwg_upsample_nearest_backward": "test_upsample_nearest",
    "pwg_tade_modulate_forward": "test_tade_modulate",
    "pwg_tade_modulate_backward": "test_tade_modulate",
    "pwg_softmax_gate_forward": "test_gates",
    "pwg_softmax_gate_backward": "test_gates",
    "pwg_copy_channels": "test_copy_channels",
    "pwg_dropout": "tests/test_uhifigan_gpu.py",
    "pwg_reduce_forward": "test_reduce",
    "pwg_reduce_backward": "test_reduce",
    "pwg_multi_reduce_forward": "test_multi_reduce",
    "pwg_multi_reduce_backward": "test_multi_reduce",
}


# ------------------------------------------------------------------------------------------------------ machinery
def _randn(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _gpu(device, fn, ins, req, dy=None):
    """``fn`` and its gradients on the device, twice, each time under ``poison_empty``; the two runs bit-equal."""
    runs = []
    for _ in range(2):
        with poison_empty():
            xs = [None if t is None else t.to(device).requires_grad_(bool(r)) for t, r in zip(ins, req)]
            y = fn(*xs)
            gs = ()
            if dy is not None and any(req):
                gs = torch.autograd.grad(y, [x for x, r in zip(xs, req) if r], dy.to(device))
        runs.append([y.detach().cpu()] + [g.cpu() for g in gs])
    for i, (a, b) in enumerate(zip(*runs)):
        assert not torch.isnan(a).any(), f"output {i}: {int(torch.isnan(a).sum())} elements nobody wrote (or NaN)"
        assert torch.equal(a, b), f"output {i} differs between two runs"
    return runs[0]


def _bits(op, got, ref):
    want = ref.to(got.dtype)
    assert got.shape == want.shape, (op, got.shape, want.shape)
    assert torch.equal(got, want), f"{op}: {int((got != want).sum())} of {got.numel()} elements differ from the reference"
    print(f"{op}: bit-equal")


def _bounded(op, got, ref, bound):
    assert got.shape == ref.shape, (op, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{op}: non-finite result"
    err = (got.double() - ref).abs()
    ratio = torch.where(err > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err)).max().item() if err.numel() else 0.0
    print(f"{op}: err/bound {ratio:.3f}")
    bad = err > bound
    assert not bad.any(), (f"{op}: {int(bad.sum())} elements over the bound, worst err/bound {ratio:.3g} "
                           f"(err {err[bad].max().item():.3e})")


def _sum(op, got, ref, big_s, n_terms):
    _bounded(op, got, ref, (n_terms + 4) * R.U * big_s.double().expand_as(ref))


def _meas(op, got, ref, cpu32):
    e32 = (cpu32.double() - ref).abs().max().item() if ref.numel() else 0.0
    _bounded(op, got, ref, 4 * e32 + 4 * R.ulp32(ref))


def _compare(op, device, gpu_fn, ref_fn, ins, req, dy, kinds, abs_fn=None):
    """Forward and gradients of ``gpu_fn`` against ``ref_fn``; ``kinds[i]`` says how output ``i`` of
    ``[y, grads of the inputs flagged in req...]`` is compared.  Returns the device results."""
    names = ["y"] + [f"d_in{i}" for i, r in enumerate(req) if r]
    got = _gpu(device, gpu_fn, ins, req, dy)
    ref = R.run(ref_fn, ins, req, dy)
    assert len(got) == len(ref) == len(kinds), (len(got), len(ref), len(kinds))
    c32 = R.run(ref_fn, ins, req, dy, torch.float32) if "meas" in kinds else None
    big = R.run_abs(abs_fn or ref_fn, ins, req, dy) if any(isinstance(k, tuple) for k in kinds[1:]) else None
    for i, kind in enumerate(kinds):
        r = ref[i][0] if isinstance(ref[i], tuple) else ref[i]
        what = f"{op} {names[i]}"
        if kind == "bits":
            _bits(what, got[i], r)
        elif kind == "meas":
            c = c32[i][0] if isinstance(c32[i], tuple) else c32[i]
            _meas(what, got[i], r, c)
        else:
            s = ref[0][1] if i == 0 else big[i]
            _sum(what, got[i], r, s, kind[1])
    return got


def _off4(t):
    """An uninitialised (NaN) view of ``t``'s shape that starts 4 bytes past a 16-byte boundary."""
    buf = torch.full((t.numel() + 1,), float("nan"), dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    assert v.data_ptr() % 16 == 4
    return v


# ------------------------------------------------------------------------------------------------------ pooling
def _check_pool(device, x, k, s, p, cip):
    t_out = R.avg_pool_t_out(x.shape[-1], k, s, p)
    dy = _randn(*x.shape[:-1], t_out, seed=1)
    return _compare(f"avg_pool k{k} s{s} p{p} cip{int(cip)} t{x.shape[-1]}", device,
                    lambda v: Fn.AvgPool1dFn.apply(v, k, s, p, cip), lambda v: R.avg_pool1d(v, k, s, p, cip),
                    [x], [True], dy, [("sum", k), ("sum", k)])


def _pool_lengths(k, s, p):
    """The smallest ``t_in`` of each kind: below ``k``; the last window cut by the right padding (it ends past
    ``t_in``: only with p > 0); the last window ending exactly at ``t_in + p``; one that does neither; and a longer
    odd one."""
    kinds = {}
    for t_in in range(1, 4 * k + 4 * s):
        t_out = R.avg_pool_t_out(t_in, k, s, p)
        if t_out < 1:
            continue
        end = (t_out - 1) * s - p + k
        for name, hit in (("short", t_in < k), ("cut", end > t_in), ("flush", end == t_in + p and t_in >= k),
                          ("slack", end < t_in + p and t_in >= k)):
            if hit:
                kinds.setdefault(name, t_in)
    return sorted(set(kinds.values()) | {3 * k + 2 * s + 1})


@pytest.mark.gpu
@pytest.mark.parametrize("cip", [True, False])
@pytest.mark.parametrize("k,s,p", [(4, 2, 2), (4, 2, 0), (3, 1, 1), (1, 1, 0), (5, 3, 2), (2, 3, 0), (7, 2, 3)])
def test_avg_pool(k, s, p, cip, device):
    lengths = _pool_lengths(k, s, p)
    assert len(lengths) >= (2 if k == 1 else 3), lengths
    for t_in in lengths:
        x = _randn(1, 3, t_in, seed=t_in)
        _, dx = _check_pool(device, x, k, s, p, cip)
        if s > k:  # inputs between the windows, and past the last one, lie in no window: their gradient is exactly 0
            t_out = R.avg_pool_t_out(t_in, k, s, p)
            covered = torch.zeros(t_in, dtype=torch.bool)
            for o in range(t_out):
                covered[max(o * s - p, 0):o * s - p + k] = True
            assert not covered.all() or t_in <= k
            assert (dx[..., ~covered] == 0).all() and (dx[..., covered] != 0).all()


# A window of the floor-mode geometry above never passes t_in + p, so the clip of the divisor at t_in + p is only met
# when the caller asks for torch's ceil_mode window count: the entry points take t_out as given.
@pytest.mark.gpu
@pytest.mark.parametrize("cip", [True, False])
@pytest.mark.parametrize("k,s,p,t_in", [(4, 2, 2, 5), (5, 3, 2, 6), (7, 2, 3, 8), (2, 3, 0, 4)])
def test_avg_pool_window_past_the_right_padding(k, s, p, t_in, cip, device):
    t_out = R.avg_pool_t_out(t_in, k, s, p, ceil_mode=True)
    assert t_out == R.avg_pool_t_out(t_in, k, s, p) + 1 and (t_out - 1) * s - p + k > t_in + p
    x, dy = _randn(1, 3, t_in, seed=t_in), _randn(1, 3, t_out, seed=t_in + 1)
    runs = []
    for _ in range(2):
        with poison_empty():
            xd, dyd = x.to(device), dy.to(device)
            y, dx = torch.empty_like(dyd), torch.empty_like(xd)
            _lib.check(_lib.lib().pwg_avg_pool1d_forward(_ptr(xd), _ptr(y), 3, t_in, t_out, k, s, p, int(cip), _stream()),
                       "avg_pool1d_forward")
            _lib.check(_lib.lib().pwg_avg_pool1d_backward(_ptr(dyd), _ptr(dx), 3, t_in, t_out, k, s, p, int(cip), _stream()),
                       "avg_pool1d_backward")
        runs.append((y.cpu(), dx.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    fn = lambda v: R.avg_pool1d(v, k, s, p, cip, ceil_mode=True)
    ref, big = R.run(fn, [x], [True], dy), R.run_abs(fn, [x], [True], dy)
    op = f"avg_pool ceil k{k} s{s} p{p} cip{int(cip)} t{t_in}"
    _sum(op + " y", runs[0][0], ref[0][0], ref[0][1], k)
    _sum(op + " dx", runs[0][1], ref[1], big[1], k)


# ------------------------------------------------------------------------------------------------------ padding
def _check_pad(device, x, pl, pr, mode):
    t_in = x.shape[-1]
    dy = _randn(*x.shape[:-1], t_in + pl + pr, seed=2)
    bwd = {"zero": "bits", "reflect": ("sum", 3), "replicate": ("sum", max(pl, pr) + 1)}[mode]
    return _compare(f"pad {mode} ({pl},{pr}) t{t_in}", device, lambda v: Fn.Pad1dFn.apply(v, pl, pr, mode),
                    lambda v: R.pad1d(v, pl, pr, mode), [x], [True], dy, ["bits", bwd])


def _pads(mode, t_in):
    pads = [(0, 0), (3, 0), (0, 5), (2, 7), (t_in - 1, t_in - 1)]
    if mode == "replicate":
        pads += [(t_in + 3, 2 * t_in + 1)]
    # reflect: pwg_pad1d_forward's PWG_REQUIRE(pad_left < t_in && pad_right < t_in) refuses the others (the mirror of
    # a signal is only defined up to one signal length): they are asserted to be refused below, not run
    return [pd for pd in pads if mode != "reflect" or max(pd) < t_in]


@pytest.mark.gpu
@pytest.mark.parametrize("t_in", [1, 2, 9, 300])
@pytest.mark.parametrize("mode", ["zero", "reflect", "replicate"])
def test_pad(mode, t_in, device):
    pads = _pads(mode, t_in)
    assert pads or (mode == "reflect" and t_in == 1)
    for pl, pr in pads:
        _check_pad(device, _randn(5, t_in, seed=pl + 10 * pr), pl, pr, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("t_in,pl,pr", [(1, 1, 0), (2, 2, 0), (9, 0, 9), (9, 12, 3)])
def test_reflect_pad_not_smaller_than_the_input_is_refused(t_in, pl, pr, device):
    x = _randn(5, t_in).to(device)
    y = torch.full((5, t_in + pl + pr), 7.0, device=device)
    rc = _lib.lib().pwg_pad1d_forward(_ptr(x), _ptr(y), 5, t_in, pl, pr, _lib.PWG_PAD_REFLECT, _stream())
    assert rc != 0 and b"reflect padding" in _lib.lib().pwg_last_error()
    assert (y == 7.0).all(), "the refused call launched"
    with pytest.raises(RuntimeError, match="reflect padding"):
        Fn.Pad1dFn.apply(x, pl, pr, "reflect")


# ------------------------------------------------------------------------------------------------------ frame fold
@pytest.mark.gpu
@pytest.mark.parametrize("t,pad,hop,n_cols", [
    (21, 8, 4, 10),    # hop does not divide t; the last frames read the right mirror
    (20, 19, 3, 25),   # pad = t - 1: the whole left mirror; frames past one reflection read zero
    (20, -5, 4, 3),    # pad < 0: the fold starts inside the signal
    (20, -5, 7, 9),    # pad < 0 and frames that run through the right mirror into the zeros
    (7, 6, 5, 8),      # every position further than one reflection: mostly zeros
    (2, 1, 1, 6),      # the shortest signal that has a mirror
])
def test_frame_fold(t, pad, hop, n_cols, device):
    x, dy = _randn(3, t, seed=t), _randn(3, hop, n_cols, seed=pad + 100)
    y, _ = _compare(f"frame_fold t{t} pad{pad} hop{hop} n{n_cols}", device,
                    lambda v: Fn.FrameFoldFn.apply(v, pad, hop, n_cols), lambda v: R.frame_fold(v, pad, hop, n_cols),
                    [x], [True], dy, ["bits", ("sum", 3)])
    if n_cols * hop - pad > 2 * t - 1:
        assert (y.reshape(3, -1)[:, -1] == 0).all()  # the last folded position lies past one reflection


# ------------------------------------------------------------------------------------------------------ floors
@pytest.mark.gpu
@pytest.mark.parametrize("eps,planted", [(2.0 ** -20, True), (R.f32(1e-7), False)])
def test_stft_mag(eps, planted, device):
    """``sqrt(max(re^2 + im^2, eps))``.  With eps = 2^-20 the planted elements have a power that float32 and float64
    both form exactly: below the floor (2^-21), AT it (2^-20 + 0) and above it (2^-19)."""
    spec = _randn(2, 6, 7, seed=3, scale=1e-3 if planted else 1.0)
    if planted:
        for col, (re, im) in enumerate([(2.0 ** -11, 2.0 ** -11), (2.0 ** -10, 0.0), (2.0 ** -10, 2.0 ** -10), (0.0, 0.0)]):
            spec[:, :3, col], spec[:, 3:, col] = re, im
    dmag = _randn(2, 3, 7, seed=4)
    _, dspec = _compare(f"stft_mag eps{eps:.1e}", device, lambda v: Fn.StftMagFn.apply(v, eps), lambda v: R.stft_mag(v, eps),
                        [spec], [True], dmag, ["meas", "meas"])
    if planted:
        assert (dspec[:, :, 0] == 0).all() and (dspec[:, :, 3] == 0).all(), "gradient below the floor"
        assert (dspec[:, :3, 1] != 0).all(), "no gradient AT the floor (torch.clamp passes it)"


@pytest.mark.gpu
@pytest.mark.parametrize("log_div", [1.0, R.f32(math.log(2.0)), R.f32(math.log(10.0))])
def test_log_clamp(log_div, device):
    eps = R.f32(1e-5)
    x = _randn(5, 61, seed=5).abs() * 1e-4
    x[:, 0], x[:, 1], x[:, 2], x[:, 3], x[:, 4] = eps, eps / 2, eps * 2, 0.0, -1.0
    dy = _randn(5, 61, seed=6)
    _, dx = _compare(f"log_clamp div{log_div:.3f}", device, lambda v: Fn.LogClampFn.apply(v, eps, log_div),
                     lambda v: R.log_clamp(v, eps, log_div), [x], [True], dy, ["meas", "meas"])
    assert (dx[:, [1, 3, 4]] == 0).all(), "gradient below the floor"
    assert (dx[:, 0] != 0).all(), "no gradient AT the floor (torch.clamp passes it)"


# ------------------------------------------------------------------------------------------------------ gates
def _check_gate(device, which, z, seed=7):
    c = z.shape[1] // 2
    dy = _randn(z.shape[0], c, z.shape[2], seed=seed)
    gpu_fn, ref_fn = {
        "gate": (lambda v: Fn.GateFn.apply(v), R.gate),
        "softmax": (lambda v: Fn.SoftmaxGateFn.apply(v, True), lambda v: R.tade_gate(v, True)),
        "sigmoid": (lambda v: Fn.SoftmaxGateFn.apply(v, False), lambda v: R.tade_gate(v, False)),
    }[which]
    op = f"{which if which == 'gate' else which + '_gate'} c{c} t{z.shape[2]} max{z.abs().max().item():.0f}"
    return _compare(op, device, gpu_fn, ref_fn, [z], [True], dy, ["meas", "meas"])


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("c,t", list(itertools.product([1, 3, 12], [1, 77])))
@pytest.mark.parametrize("which", ["gate", "softmax", "sigmoid"])
def test_gates(which, c, t, scale, device):
    z = _randn(3, 2 * c, t, seed=c + t, scale=scale)
    if scale > 1:  # +-90: exp(90) overflows float32, a softmax without the max subtraction would give inf / inf
        z = z.clamp(-90.0, 90.0)
        z[0, :, 0] = 90.0
        z[1, :, 0] = -90.0
        z[2, ::2, 0], z[2, 1::2, 0] = 90.0, -90.0
    _check_gate(device, which, z)


def _check_modulate(device, xn, cg, s, req=(True, True)):
    b, c, t = xn.shape
    dy = _randn(b, c, t * s, seed=8)
    kinds = [("sum", 2)] + ([("sum", s)] if req[0] else []) + (["bits"] if req[1] else [])
    return _compare(f"tade_modulate c{c} t{t} s{s} req{int(req[0])}{int(req[1])}", device,
                    lambda a, g: Fn.TadeModulateFn.apply(a, g, s), lambda a, g: R.tade_modulate(a, g, s), [xn, cg],
                    list(req), dy, kinds)


@pytest.mark.gpu
@pytest.mark.parametrize("c,t", list(itertools.product([1, 3, 12], [1, 77])))
def test_tade_modulate(c, t, device):
    for s in (1, 2, 5):
        xn, cg = _randn(3, c, t, seed=s), _randn(3, 2 * c, t * s, seed=s + 10)
        for req in ((True, True), (True, False), (False, True)):  # both, dxn only, dcg only
            _check_modulate(device, xn, cg, s, req)


def _check_upsample(device, x, s, add):
    dy = _randn(*x.shape[:-1], x.shape[-1] * s, seed=9)
    if add is None:
        return _compare(f"upsample s{s}", device, lambda v: Fn.UpsampleNearestFn.apply(v, s),
                        lambda v: R.upsample_nearest(v, s), [x], [True], dy, ["bits", ("sum", s)])
    # x + add is ONE correctly rounded addition: bit-equal as well
    return _compare(f"upsample s{s} +add", device, lambda v, a: Fn.UpsampleNearestFn.apply(v, s, a),
                    lambda v, a: R.upsample_nearest(v, s, a), [x, add], [True, True], dy, ["bits", ("sum", s), "bits"])


@pytest.mark.gpu
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("s", [1, 3, 8])
def test_upsample_nearest(s, with_add, device):
    for t in (1, 11):
        _check_upsample(device, _randn(1, 5, t, seed=s), s, _randn(1, 5, t * s, seed=s + 1) if with_add else None)


# ------------------------------------------------------------------------------------------------------ stretch-conv
ACTS = (None, "leaky_relu", "relu", "tanh")
# every (s, F, centred / causal) of s in 1..4, F in 1, 3, 5 passes stretch_conv_check (kernel = 2 s + 1 <= 64,
# pad_left = s or 2 s < kernel, F odd <= 15): nothing is removed.  The activation cycles so that the set covers all four
# with every s and every F.
STRETCH = [(s, fk, causal, ACTS[(i + i // 4) % 4])
           for i, (s, fk, causal) in enumerate(itertools.product([1, 2, 3, 4], [1, 3, 5], [False, True]))]


def _stretch_raw(x, w, y, s, pad_left, act):
    (b, c, t_in), (fk, k) = x.shape, w.shape
    _lib.check(_lib.lib().pwg_stretch_conv_forward(_ptr(x), _ptr(w), _ptr(y), b * c, t_in, s, k, pad_left, c, fk,
                                                   ops.ACT[act], SLOPE, _stream()), "stretch_conv_forward")


def _check_stretch(device, x, w, s, pad_left, act):
    (b, c, t_in), (fk, k) = x.shape, w.shape
    dy = _randn(b, c, t_in * s, seed=10)
    if act == "tanh":
        kinds = ["meas", "meas", "meas"]
    else:  # the weight gradient sums over every output position of every row
        kinds = [("sum", fk * k), ("sum", fk * k * s), ("sum", b * c * t_in * s)]
    op = f"stretch_conv s{s} F{fk} pad{pad_left} {act} t{t_in}"
    got = _compare(op, device, lambda v, u: Fn.StretchConvFn.apply(v, u, s, pad_left, act, SLOPE),
                   lambda v, u: R.stretch_conv(v, u, s, pad_left, act, SLOPE), [x, w], [True, True], dy, kinds,
                   abs_fn=lambda v, u: R.stretch_conv(v, u, s, pad_left))
    if fk == 1 and pad_left == s and s in (2, 4) and (t_in * s) % 4 == 0:
        # the 4-outputs-per-thread kernel ran above (aligned output); an output view one float off a 16-byte boundary
        # makes the generic kernel run: "same products in the same tap order (bit-identical)"
        xd, wd = x.to(device), w.to(device)
        y4 = torch.full((b, c, t_in * s), float("nan"), device=device)
        assert y4.data_ptr() % 16 == 0
        yg = _off4(y4)
        _stretch_raw(xd, wd, y4, s, pad_left, act)
        _stretch_raw(xd, wd, yg, s, pad_left, act)
        assert torch.equal(y4.cpu(), got[0]), "direct call differs from StretchConvFn"
        assert torch.equal(yg, y4), f"{op}: fwd4 differs from the generic kernel in {int((yg != y4).sum())} elements"
        print(f"{op}: fwd4 == generic")
        return True
    return False


@pytest.mark.gpu
@pytest.mark.parametrize("s,fk,causal,act", STRETCH)
def test_stretch_conv(s, fk, causal, act, device):
    assert {a for _, _, _, a in STRETCH} == set(ACTS)
    compared = [_check_stretch(device, _randn(2, 3, t_in, seed=t_in), _randn(fk, 2 * s + 1, seed=fk + s),
                               s, 2 * s if causal else s, act) for t_in in (1, 2, 13)]
    assert any(compared) == (fk == 1 and not causal and s in (2, 4))


# ------------------------------------------------------------------------------------------------------ norms
@pytest.mark.gpu
@pytest.mark.parametrize("t", [1, 2, 63, 255, 256, 257, 1000])
def test_instance_norm(t, device):
    x, dy = _randn(1, 5, t, seed=t), _randn(1, 5, t, seed=t + 1)
    y, dx = _compare(f"instance_norm t{t}", device, lambda v: Fn.InstanceNormFn.apply(v, EPS_NORM),
                     lambda v: R.instance_norm(v, EPS_NORM), [x], [True], dy, ["meas", "meas"])
    if t == 1:  # zero variance: x - mean is exactly 0, and so is dy - mean(dy)
        assert (y == 0).all() and (dx == 0).all()


@pytest.mark.gpu
def test_instance_norm_of_a_large_offset(device):
    """x = 1000 + 0.01 noise: the mean is known to ~1e-4 in float32, 1 % of the spread.  The bar is what torch's own
    float32 evaluation loses here, not a wider one."""
    x, dy = 1000.0 + 0.01 * _randn(1, 5, 257, seed=11), _randn(1, 5, 257, seed=12)
    _compare("instance_norm offset 1000", device, lambda v: Fn.InstanceNormFn.apply(v, EPS_NORM),
             lambda v: R.instance_norm(v, EPS_NORM), [x], [True], dy, ["meas", "meas"])


@pytest.mark.gpu
@pytest.mark.parametrize("inner", [1, 63, 64, 255, 256, 257, 1000])
@pytest.mark.parametrize("n0", [1, 5])
def test_weight_norm(n0, inner, device):
    v, g, dw = _randn(n0, inner, seed=inner), _randn(n0, 1, seed=n0), _randn(n0, inner, seed=inner + 1)
    g[0] = -abs(g[0]) - 0.5          # a negative gain
    if n0 > 1:
        g[1], g[2] = 0.0, abs(g[2]) + 0.5  # a gain of exactly zero
    _compare(f"weight_norm n0 {n0} inner {inner}", device, lambda a, b: Fn.WeightNormFn.apply(a, b), R.weight_norm,
             [v, g], [True, True], dw, ["meas", "meas", "meas"])
    # the stand-alone backward kernel alone, on the same data
    outs = []
    for _ in range(2):
        with poison_empty():
            d = [t.to(device) for t in (dw, v, g)]
            o = [torch.empty_like(d[1]), torch.empty_like(d[2])]
            _lib.check(_lib.lib().pwg_weight_norm_backward(_ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(o[0]), _ptr(o[1]), n0,
                                                           inner, _stream()), "weight_norm_backward")
        outs.append([t.cpu() for t in o])
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    ref = R.run(R.weight_norm, [v, g], [True, True], dw)
    c32 = R.run(R.weight_norm, [v, g], [True, True], dw, torch.float32)
    _meas(f"weight_norm_backward n0 {n0} inner {inner} dv", outs[0][0], ref[1], c32[1])
    _meas(f"weight_norm_backward n0 {n0} inner {inner} dg", outs[0][1], ref[2], c32[2])


def _check_spectral(device, w, u0, v0, do_iter, eps=1e-12):
    rows, cols = w.shape
    op = f"spectral_norm ({rows},{cols}) iter{int(do_iter)}"
    dy = _randn(rows, cols, seed=13)
    runs = []
    for _ in range(2):
        with poison_empty():
            wd, u, v = w.to(device).requires_grad_(True), u0.to(device), v0.to(device)
            y = Fn.SpectralNormFn.apply(wd, u, v, do_iter, eps)
            _, u_saved, v_saved, sigma = y.grad_fn.saved_tensors
            (dw,) = torch.autograd.grad(y, wd, dy.to(device))
        runs.append([t.detach().cpu() for t in (y, dw, sigma.reshape(()), u, v, u_saved, v_saved)])
    for a, b in zip(*runs):
        assert not torch.isnan(a).any() and torch.equal(a, b), op
    y, dw, sigma, u, v, u_saved, v_saved = runs[0]
    fn = lambda t: R.spectral_norm(t, u0, v0, do_iter, eps)
    ref, c32 = R.run(fn, [w], [True], dy), R.run(fn, [w], [True], dy, torch.float32)
    (y_r, sigma_r, u_r, v_r), dw_r = ref
    (y_c, sigma_c, u_c, v_c), dw_c = c32
    for name, got, r, c in (("w", y, y_r, y_c), ("dw", dw, dw_r, dw_c), ("sigma", sigma, sigma_r, sigma_c),
                            ("u", u, u_r, u_c), ("v", v, v_r, v_c)):
        _meas(f"{op} {name}", got, r, c)
    assert torch.equal(u_saved, u) and torch.equal(v_saved, v), "the saved copies are not this forward's u, v"
    if not do_iter:
        assert torch.equal(u, u0) and torch.equal(v, v0), "u, v changed without an iteration"


def _power_vectors(w, iters=30):
    """Unit vectors near the leading singular pair (what the buffers hold after some training steps)."""
    u = torch.nn.functional.normalize(_randn(w.shape[0], seed=14).double(), dim=0)
    for _ in range(iters):
        v = torch.nn.functional.normalize(w.double().t() @ u, dim=0)
        u = torch.nn.functional.normalize(w.double() @ v, dim=0)
    return u.float(), v.float()


@pytest.mark.gpu
@pytest.mark.parametrize("do_iter", [True, False])
@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 65), (3, 63), (65, 1), (65, 130), (130, 257)])
def test_spectral_norm(rows, cols, do_iter, device):
    w = _randn(rows, cols, seed=rows + cols)
    _check_spectral(device, w, *_power_vectors(w, iters=3), do_iter)


# ------------------------------------------------------------------------------------------------------ small ones
def _check_act_backward(device, n, act, scale):
    dy, y = _randn(n, seed=15), torch.tanh(_randn(n, seed=16))
    y[0], y[1], y[2 % n] = 0.0, -0.0, 0.0
    outs = []
    for _ in range(2):
        with poison_empty():
            d_dy, d_y = dy.to(device), y.to(device)
            dx = torch.empty_like(d_dy)
            _lib.check(_lib.lib().pwg_act_backward(_ptr(d_dy), _ptr(d_y), _ptr(dx), n, ops.ACT[act], SLOPE, scale,
                                                   _stream()), "act_backward")
        outs.append(dx.cpu())
    assert torch.equal(outs[0], outs[1])
    ref = R.act_backward(dy.double(), y.double(), act, SLOPE, scale)
    if act == "tanh":
        _meas(f"act_backward {act}", outs[0], ref, R.act_backward(dy, y, act, SLOPE, scale))
    else:
        _bits(f"act_backward {act}", outs[0], ref)


# leaky_relu multiplies twice (dy * scale, then * slope): a power-of-two scale keeps the first product exact, so the
# result is still ONE rounding of the float64 value; the other activations get a scale with a full mantissa
@pytest.mark.gpu
@pytest.mark.parametrize("act,scale", [(None, R.f32(0.3)), ("leaky_relu", 0.5), ("relu", R.f32(0.3)), ("tanh", R.f32(0.3))])
def test_act_backward(act, scale, device):
    for n in (3, 257):
        _check_act_backward(device, n, act, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("with_c", [False, True])
def test_add3_div(with_c, device):
    a, b, c, dy = (_randn(3, 5, 61, seed=s) for s in (17, 18, 19, 20))
    if with_c:
        _compare("add3_div a b c", device, lambda p, q, r: Fn.Add3DivFn.apply(p, q, r, 3.0),
                 lambda p, q, r: R.add3_div(p, q, r, 3.0), [a, b, c], [True, True, True], dy, ["meas"] * 4)
    else:
        _compare("add3_div a b", device, lambda p, q: Fn.Add3DivFn.apply(p, q, None, 3.0),
                 lambda p, q: R.add3_div(p, q, None, 3.0), [a, b], [True, True], dy, ["meas"] * 3)


def _check_pcm(device, x):
    outs = []
    for _ in range(2):
        with poison_empty():
            outs.append(streaming.to_pcm16(x.to(device)).cpu())
    assert torch.equal(outs[0], outs[1])
    _bits("wave_to_pcm16", outs[0], R.wave_to_pcm16(x))


@pytest.mark.gpu
def test_wave_to_pcm16(device):
    ms = list(range(-40, 40)) + [1000, 1001, -1000, -1001, 32765, 32766, -32766, -32767]
    half = torch.tensor([(m + 0.5) / 32767 for m in ms], dtype=torch.float64).float()
    prod = half.numpy() * np.float32(32767)
    exact = [m for m, p in zip(ms, prod) if p == m + 0.5]  # the float32 product IS half-way: round to even decides
    assert sum(m % 2 == 0 for m in exact) >= 5 and sum(m % 2 == 1 for m in exact) >= 5, exact
    edge = torch.tensor([1.0, -1.0, 1.5, -1.5, 0.0, -0.0, 2.0 ** -149, -2.0 ** -149, 1e30, -1e30, float("inf"),
                         -float("inf")])
    _check_pcm(device, torch.cat([half, edge, _randn(300, seed=21, scale=0.6)]))


def _check_normalize_transpose(device, x, mean, scale):
    outs = []
    for _ in range(2):
        with poison_empty():
            args = [None if t is None else t.to(device) for t in (x, mean, scale)]
            outs.append(streaming.normalize_transpose(*args).cpu())
    assert torch.equal(outs[0], outs[1])
    op = f"normalize_transpose {tuple(x.shape)} stats{int(mean is not None)}"
    if mean is None:
        return _bits(op, outs[0], R.normalize_transpose(x.double()))
    _meas(op, outs[0], R.normalize_transpose(x.double(), mean.double(), scale.double()),
          R.normalize_transpose(x, mean, scale))


@pytest.mark.gpu
@pytest.mark.parametrize("channels,frames", list(itertools.product([1, 80], [1, 33])))
def test_normalize_transpose(channels, frames, device):
    x = _randn(3, frames, channels, seed=22)
    _check_normalize_transpose(device, x, None, None)
    _check_normalize_transpose(device, x, _randn(channels, seed=23), _randn(channels, seed=24).abs() + 0.5)


def _check_copy_channels(device, a, b):
    """``ConcatChannelsFn``: forward = pwg_copy_channels at c_off 0 and at c_off = c_dst - c_src, backward = the same two
    in the reverse direction."""
    dy = _randn(a.shape[0], a.shape[1] + b.shape[1], a.shape[2], seed=25)
    _compare(f"copy_channels {a.shape[1]}+{b.shape[1]}", device, lambda p, q: Fn.ConcatChannelsFn.apply(p, q),
             R.concat_channels, [a, b], [True, True], dy, ["bits", "bits", "bits"])


@pytest.mark.gpu
@pytest.mark.parametrize("ca,cb,t", [(3, 5, 7), (1, 1, 1), (5, 2, 77)])
def test_copy_channels(ca, cb, t, device):
    _check_copy_channels(device, _randn(3, ca, t, seed=26), _randn(3, cb, t, seed=27))


# ------------------------------------------------------------------------------------------------------ reductions
def _tie_data(n, seed):
    """Random operands with the ties planted in front: a == b (also at +-1 and 0), one operand exactly 0 (also -0.0),
    the hinge arguments exactly +-1."""
    a, b = _randn(n, seed=seed), _randn(n, seed=seed + 1)
    ties = [(1, 1), (-1, -1), (0, 0), (0, 0.5), (0.5, 0), (-0.0, 0.3), (1, -1), (-1, 1)]
    if n >= len(ties):
        for i, (x, y) in enumerate(ties):
            a[i], b[i] = x, y
    return a, b


def _reduce_kinds(mode, n):
    return 2 * n if mode == "abs_diff_lrelu" else n


def _check_grad(op, got, ref):
    # gout * scale, times the derivative: at most three roundings of products, no sum -> 4 * 2^-24 relative; a
    # reference of exactly 0 (a tie, or the flat side of the hinge) allows nothing
    _bounded(op, got, ref, 4 * R.U * ref.abs())


# reduce_stage1_kernel's launcher caps the grid at RED_BLOCKS = 512 workgroups of 256 threads: 131 072 threads.
# n = 131 072 + 77 is past one such grid (with its (n + 1023) / 1024 = 129 workgroups every thread takes several
# trips of the stride loop, the last one ragged); reduce_backward_kernel's 4096-workgroup cap is met by
# test_second_trip_of_the_stride_loop.
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 257, 131072 + 77])
@pytest.mark.parametrize("mode", R.RED_MODES)
def test_reduce(mode, n, device):
    a, b = _tie_data(n, seed=n % 1000)
    binary = mode in R.RED_BINARY
    c, scale, gout = 0.25, R.f32(1.0 / n), torch.tensor(0.75)
    reqs = [(True, True), (True, False), (False, True)] if binary else [(True, False)]
    for req in reqs:
        ins = [a, b if binary else None]
        got = _gpu(device, lambda p, q: Fn.ReduceFn.apply(p, q, mode, scale, c), ins, req, gout)
        val, big_s = R.reduce_value(mode, a.double(), b.double(), c, scale)
        op = f"reduce {mode} n{n} req{int(req[0])}{int(req[1])}"
        _sum(op, got[0], val, big_s, _reduce_kinds(mode, n))
        grads = [g for g, r in zip(R.reduce_grads(mode, a.double(), b.double(), c, scale, 0.75), req) if r]
        assert len(grads) == len(got) - 1
        for g, r in zip(got[1:], grads):
            _check_grad(op + " grad", g, r)


@pytest.mark.gpu
def test_multi_reduce(device):
    """All eight modes in one launch pair, two slots, the same ties; two items longer than one 8192-element chunk."""
    c, gout = 0.25, torch.tensor([0.75, -1.5])
    spec, tensors, req = [], [], []
    for i, mode in enumerate(R.RED_MODES):
        n = 8192 + 77 if i in (1, 6) else 257
        a, b = _tie_data(n, seed=30 + 2 * i)
        spec.append((mode, R.f32(1.0 / (n + i)), c, i % 2))
        tensors += [a, b if mode in R.RED_BINARY else None]
        req += [True, mode in R.RED_BINARY]
    got = _gpu(device, lambda *ts: Fn.MultiReduceFn.apply(spec, 2, *ts), tensors, req, gout)
    val, big_s, terms = torch.zeros(2, dtype=D), torch.zeros(2, dtype=D), [0, 0]
    grads = []
    for i, (mode, scale, _, slot) in enumerate(spec):
        a, b = tensors[2 * i].double(), None if tensors[2 * i + 1] is None else tensors[2 * i + 1].double()
        v, s = R.reduce_value(mode, a, b, c, scale)
        val[slot] += v
        big_s[slot] += s
        terms[slot] += _reduce_kinds(mode, a.numel())
        grads += [g for g in R.reduce_grads(mode, a, b, c, scale, gout[slot].item()) if g is not None]
    _sum("multi_reduce", got[0], val, big_s, max(terms))
    assert len(grads) == len(got) - 1
    for i, (g, r) in enumerate(zip(got[1:], grads)):
        _check_grad(f"multi_reduce grad {i}", g, r)


# ------------------------------------------------------------------------------------------------------ second trip
# grid_for caps a launch at 4096 workgroups of 256 threads = 1 048 576 threads; everything past that is the second trip
# of the grid-stride loop.  8006 rows of 131 elements are 1 048 786 = 1 048 576 + 210 (no multiple of 256), and row
# 8005 starts at element 1 048 655: a row boundary inside the second trip, for every kernel that splits its index into
# (row, position).  Where forward and backward launch over different tensors, both exceed one grid.
BIG_ROWS, BIG_T = 8006, 131


def _big_pool(device):
    _check_pool(device, _randn(1, BIG_ROWS, BIG_T, seed=40), 3, 1, 1, True)


def _big_pad(device):
    _check_pad(device, _randn(BIG_ROWS, BIG_T, seed=41), 2, 3, "reflect")


def _big_upsample(device):
    _check_upsample(device, _randn(1, BIG_ROWS, BIG_T, seed=42), 2, _randn(1, BIG_ROWS, 2 * BIG_T, seed=43))


def _big_modulate(device):
    _check_modulate(device, _randn(2, BIG_ROWS // 2, BIG_T, seed=44), _randn(2, BIG_ROWS, 2 * BIG_T, seed=45), 2)


def _big_gate(device):
    _check_gate(device, "gate", _randn(2, BIG_ROWS, BIG_T, seed=46))


def _big_softmax_gate(device):  # one thread per (batch, time) column
    _check_gate(device, "softmax", _randn(BIG_ROWS, 4, BIG_T, seed=47))


def _big_stretch(device):  # fwd4 (1 048 786 threads), the generic kernel (4 of them per fwd4 thread), the data gradient
    assert _check_stretch(device, _randn(2, BIG_ROWS // 2, BIG_T, seed=48), _randn(1, 9, seed=49), 4, 4, "leaky_relu")


def _big_normalize_transpose(device):
    _check_normalize_transpose(device, _randn(1, BIG_T, BIG_ROWS, seed=50), _randn(BIG_ROWS, seed=51),
                               _randn(BIG_ROWS, seed=52).abs() + 0.5)


def _big_copy_channels(device):
    _check_copy_channels(device, _randn(2, BIG_ROWS // 2, BIG_T, seed=53), _randn(2, BIG_ROWS // 2, BIG_T, seed=54))


def _big_act_backward(device):
    _check_act_backward(device, BIG_ROWS * BIG_T, "leaky_relu", 0.5)


def _big_pcm(device):
    _check_pcm(device, _randn(BIG_ROWS * BIG_T, seed=55, scale=0.6))


def _big_spectral_backward(device):
    w = _randn(BIG_ROWS, BIG_T, seed=56)
    _check_spectral(device, w, *_power_vectors(w, iters=3), True)


def _big_reduce_backward(device):
    n = BIG_ROWS * BIG_T
    a, b = _tie_data(n, seed=57)
    got = _gpu(device, lambda p, q: Fn.ReduceFn.apply(p, q, "abs_diff_lrelu", 1.0, 0.25), [a, b], [True, True],
               torch.tensor(0.75))
    for g, r in zip(got[1:], R.reduce_grads("abs_diff_lrelu", a.double(), b.double(), 0.25, 1.0, 0.75)):
        _check_grad("reduce backward", g, r)


BIG = {f.__name__[len("_big_"):]: f for f in (
    _big_pool, _big_pad, _big_upsample, _big_modulate, _big_gate, _big_softmax_gate, _big_stretch,
    _big_normalize_transpose, _big_copy_channels, _big_act_backward, _big_pcm, _big_spectral_backward,
    _big_reduce_backward)}


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", sorted(BIG))
def test_second_trip_of_the_stride_loop(kernel, device):
    assert BIG_ROWS * BIG_T > 4096 * 256 and (BIG_ROWS * BIG_T) % 256 and (BIG_ROWS - 1) * BIG_T > 4096 * 256
    BIG[kernel](device)
