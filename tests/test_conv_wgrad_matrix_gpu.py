"""GPU: every case of the weight-gradient configuration matrix (tests/wgrad_cases.py; the host file pins which variant
of conv1d_wgrad_kernel and which slab finisher each case reaches) against a float64 CPU reference through autograd:
``F.conv1d`` / ``F.conv_transpose1d`` / ``F.conv2d`` of the pre-activated input, for weight-normalised cases through
``w = g * v / ||v||``.

Per case, under NaN-filled LDS and NaN-filled ``torch.empty``:
  * ``ops.conv1d_backward_weight`` with (need_dw, need_db) = (T, T), (T, F) and (F, T) -- the last is bias_grad_kernel;
  * weight-normalised cases: ``ops.conv1d_backward_weight_wn`` with and without ``need_db``;
  * a second identical call gives the same bits (the slabs are summed in a fixed order: a finisher that reads a slab
    element nobody wrote, or a kernel that leaves one unwritten, shows here or as a NaN).

Bar: RTOL = 3e-5 of the largest reference entry, the family's bound (tests/test_conv_ops_gpu.py), here against float64.
The longest reduction of the table is 131072 products ("hint_below_1"); fp32 accumulation over N random products errs by
about 6e-8 * sqrt(N) / 4 of the largest entry, 5e-6 there, while a dropped column or tap costs about 1 / sqrt(N) >= 2.8e-3.
Measured on an MI355X: the largest error of the whole table is 6.2e-7, so no case needs a bar of its own.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from parallelwavegan_amd import functional, ops
from tests import wgrad_cases as W
from tests.util import poison_empty, poison_lds

pytestmark = pytest.mark.gpu

RTOL = 3e-5


def _act(x, slope):
    if slope is None:
        return x
    return F.relu(x) if slope == 0.0 else F.leaky_relu(x, slope)


def _conv64(c, xa, w, b):
    """The case's convolution in float64 (xa already pre-activated), flat (B, C, rows * width) in and out."""
    if c["transposed"]:
        return F.conv_transpose1d(xa, w, b, stride=c["stride"], padding=c["pad"], output_padding=c["out_pad"],
                                  groups=c["groups"])
    Wd = c["width"]
    if Wd > 1:
        x4 = F.pad(xa.reshape(c["B"], c["cin"], c["t"], Wd), (0, 0, c["pad"], c["pad_right"]))
        y = F.conv2d(x4, w.unsqueeze(-1), b, stride=(c["stride"], 1), dilation=(c["dil"], 1), groups=c["groups"])
        return y.reshape(c["B"], c["cout"], -1)
    return F.conv1d(F.pad(xa, (c["pad"], c["pad_right"])), w, b, stride=c["stride"], dilation=c["dil"], groups=c["groups"])


@functools.lru_cache(maxsize=None)
def _problem(name):
    """CPU float32 inputs of a case and its float64 gradients, computed once and shared (read-only)."""
    c = W.BY_NAME[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    g_, cin, cout, k = c["groups"], c["cin"], c["cout"], c["k"]
    x = torch.randn(c["B"], cin, c["t"] * c["width"], generator=gen)
    wshape = (cin, cout // g_, k) if c["transposed"] else (cout, cin // g_, k)
    v = torch.randn(wshape, generator=gen) / (wshape[1] * k) ** 0.5
    gg = 1.0 + 0.1 * torch.randn(wshape[0], generator=gen)
    b = 0.1 * torch.randn(cout, generator=gen)
    v64, g64, b64 = v.double().requires_grad_(), gg.double().requires_grad_(), b.double().requires_grad_()
    # every case has the plain gradient dL/dw at w = v; weight-normalised ones also dv, dg at w = g * v / ||v||
    y = _conv64(c, _act(x.double(), c["slope"]), v64, b64)
    assert y.shape[-1] == W.out_rows(c) * c["width"], (y.shape, W.out_rows(c))
    dy = torch.randn(y.shape, generator=gen)
    y.backward(dy.double())
    ref = dict(dw=v64.grad.clone(), db=b64.grad.clone())
    if c["wn"]:
        v64.grad = None
        w = g64.view(-1, 1, 1) * v64 / v64.flatten(1).norm(dim=1).view(-1, 1, 1)
        _conv64(c, _act(x.double(), c["slope"]), w, None).backward(dy.double())
        ref.update(dv=v64.grad.clone(), dg=g64.grad.clone())
    return dict(x=x, dy=dy, v=v, g=gg, ref=ref)


def _check(got, ref, what):
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item() / (ref.abs().max().item() + 1e-300)
    print(f"{what}: rel-to-max error {err:.3e}")
    assert err <= RTOL, f"{what}: rel-to-max error {err:.3e} > {RTOL}"   # (NaN fails too)


@pytest.mark.parametrize("name", [c["name"] for c in W.CASES])
def test_wgrad_case(name, device):
    c = W.BY_NAME[name]
    pr = _problem(name)
    ref = pr["ref"]
    desc = W.make_desc(c)
    x, dy, v, g = (pr[n].to(device) for n in ("x", "dy", "v", "g"))
    shape = tuple(v.shape)
    with W.concurrency_hint(c["hint"]), poison_lds(), poison_empty():
        dw, db = ops.conv1d_backward_weight(desc, x, dy, shape)
        dw2, db2 = ops.conv1d_backward_weight(desc, x, dy, shape)
        dw_only, none = ops.conv1d_backward_weight(desc, x, dy, shape, need_db=False)
        none2, db_only = ops.conv1d_backward_weight(desc, x, dy, shape, need_dw=False)
        if c["wn"]:
            dv, dg, dbw = ops.conv1d_backward_weight_wn(desc, x, dy, v, g)
            dv2, dg2, dbw2 = ops.conv1d_backward_weight_wn(desc, x, dy, v, g)
            dv_nb, dg_nb, none3 = ops.conv1d_backward_weight_wn(desc, x, dy, v, g, need_db=False)
    assert none is None and none2 is None
    _check(dw, ref["dw"], f"{name} dw")
    _check(db, ref["db"], f"{name} db")
    _check(dw_only, ref["dw"], f"{name} dw (need_db=False)")
    _check(db_only, ref["db"], f"{name} db (need_dw=False: bias_grad_kernel)")
    assert torch.equal(dw, dw2) and torch.equal(db, db2), f"{name}: a repeated call gives other bits"
    if c["wn"]:
        assert none3 is None
        _check(dv, ref["dv"], f"{name} dv")
        _check(dg, ref["dg"], f"{name} dg")
        _check(dbw, ref["db"], f"{name} db (weight-norm entry)")
        _check(dv_nb, ref["dv"], f"{name} dv (need_db=False)")
        _check(dg_nb, ref["dg"], f"{name} dg (need_db=False)")
        assert torch.equal(dv, dv2) and torch.equal(dg, dg2) and torch.equal(dbw, dbw2), \
            f"{name}: a repeated weight-norm call gives other bits"


@pytest.mark.parametrize("row", [16320, 16384])
def test_conv_param_grads_row_switch(row, device):
    """functional.conv_param_grads on both sides of its ``4 * row + 256 <= 64 KiB`` switch: 16320 floats still take the
    fused finisher (its largest row buffer), 16384 the plain weight gradient + the stand-alone pwg_weight_norm_backward
    on a row longer than the fused finisher accepts.  1 x 1 layer, 8 output channels, 2 x 8 columns."""
    B, cout, t = 2, 8, 8
    gen = torch.Generator().manual_seed(row)
    x = torch.randn(B, row, t, generator=gen)
    v = torch.randn(cout, row, 1, generator=gen) / row ** 0.5
    g = 1.0 + 0.1 * torch.randn(cout, 1, 1, generator=gen)
    b = 0.1 * torch.randn(cout, generator=gen)
    dy = torch.randn(B, cout, t, generator=gen)
    v64, g64, b64 = v.double().requires_grad_(), g.double().requires_grad_(), b.double().requires_grad_()
    w = g64 * v64 / v64.flatten(1).norm(dim=1).view(-1, 1, 1)
    F.conv1d(F.leaky_relu(x.double(), 0.1), w, b64).backward(dy.double())
    desc = ops.make_conv_desc(B, row, cout, t, t, 1, pre_act="leaky_relu", pre_slope=0.1)
    fused = 4 * row + 256 <= 64 * 1024
    with poison_lds(), poison_empty(), ops.profile() as prof:
        dv, dg, db = functional.conv_param_grads(desc, x.to(device), dy.to(device), tuple(v.shape), tuple(v.shape),
                                                 v.to(device), g.to(device), True, True, True)
    assert ("reduce_slabs_wn_kernel" in prof.results) == fused, sorted(prof.results)
    _check(dv, v64.grad, f"row {row} dv")
    _check(dg, g64.grad, f"row {row} dg")
    _check(db, b64.grad, f"row {row} db")
