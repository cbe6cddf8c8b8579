"""CPU: the float64 references of tests/wavenet_refs.py against torch's own float64 evaluation and autograd of the
layer written tap by tap (so that the GPU matrix of tests/test_wavenet_matrix_gpu.py is compared with something that is
itself checked); the completeness check: every ``pwg_wavenet_*`` entry point of csrc/wavenet.hip must name, in
``COVERED``, the test that drives it directly; and the refusal table of ``pwg_wavenet_layer_supported``."""
import ctypes
import importlib
import itertools
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import wavenet_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = torch.float64
TIGHT = 1e-12  # two float64 evaluations of O(1) quantities over at most a few hundred terms (test_elementwise_refs_host.py)
AUX = 80


def _close(a, b, tol=TIGHT):
    assert a.shape == b.shape, (a.shape, b.shape)
    err = (a - b).abs().max().item()
    assert err <= tol * max(1.0, b.abs().max().item()), err


def _layer_by_taps(x, c, skips, Wd, Wa, Ws, Wo, b_dil, b_skip, b_out, dil, out_mul, skip_mul, z_leaf=None):
    """The layer with every convolution as explicit shifted matrix products (autograd-capable); ``z_leaf`` replaces the
    gate input (a leaf there gives dz)."""
    T = x.shape[-1]
    xp = F.pad(x, (dil, dil))
    z = sum(torch.einsum("oc,bct->bot", Wd[:, :, k], xp[:, :, k * dil:k * dil + T]) for k in range(3))
    z = z + torch.einsum("oc,bct->bot", Wa[:, :, 0], c)
    if b_dil is not None:
        z = z + b_dil.view(1, -1, 1)
    zz = z if z_leaf is None else z_leaf
    g = torch.tanh(zz[:, :64]) / (1 + torch.exp(-zz[:, 64:]))
    s = torch.einsum("oc,bct->bot", Ws[:, :, 0], g)
    o = torch.einsum("oc,bct->bot", Wo[:, :, 0], g)
    if b_skip is not None:
        s = s + b_skip.view(1, -1, 1)
    if b_out is not None:
        o = o + b_out.view(1, -1, 1)
    if skips is not None:
        s = s + skips
    return z, g, s * skip_mul, (o + x) * out_mul


@pytest.mark.parametrize("T", [1, 5, 65])
@pytest.mark.parametrize("dil", [1, 3, 512])
def test_references_match_torch_autograd(T, dil):
    gen = torch.Generator().manual_seed(1000 * T + dil)
    r = lambda *s: torch.randn(*s, dtype=D, generator=gen)  # noqa: E731
    B = 2
    x, c, skips_all = r(B, 64, T), r(B, AUX, T), r(B, 64, T)
    Wd, Wa = r(128, 64, 3) / math.sqrt(192), r(128, AUX, 1) / math.sqrt(AUX)
    Ws, Wo = r(64, 64, 1) / 8, r(64, 64, 1) / 8
    biases = (r(128), r(64), r(64))
    dx_out_all, ds_out, dc_accum_all = r(B, 64, T), r(B, 64, T), r(B, AUX, T)
    out_mul, skip_mul = math.sqrt(0.5), math.sqrt(1 / 30)
    for with_b, with_skips, with_dx, with_acc in itertools.product((True, False), repeat=4):
        b_dil, b_skip, b_out = biases if with_b else (None, None, None)
        skips = skips_all if with_skips else None
        dx_out = dx_out_all if with_dx else None
        dc_accum = dc_accum_all if with_acc else None
        args = (Wd, Wa, Ws, Wo, b_dil, b_skip, b_out, dil, out_mul, skip_mul)
        # forward
        xr, cr = x.clone().requires_grad_(), c.clone().requires_grad_()
        z_t, g_t, s_t, o_t = _layer_by_taps(xr, cr, skips, *args)
        z, g, s_out, x_out = R.layer_forward(x, c, skips, *args)
        for ours, theirs in ((z, z_t), (g, g_t), (s_out, s_t), (x_out, o_t)):
            _close(ours, theirs.detach())
        # backward: dz through a leaf at z, dx and dc through the whole graph (dc_accum: what a later layer that reads
        # the same aux features contributes)
        z_leaf = z.clone().requires_grad_()
        _, _, s_l, o_l = _layer_by_taps(x, c, skips, *args, z_leaf=z_leaf)
        loss = lambda s_, o_: (s_ * ds_out).sum() + ((o_ * dx_out).sum() if with_dx else 0.0)  # noqa: E731
        dz_t = torch.autograd.grad(loss(s_l, o_l), z_leaf)[0]
        total = loss(s_t, o_t) + ((cr * dc_accum).sum() if with_acc else 0.0)
        dx_t, dc_t = torch.autograd.grad(total, (xr, cr))
        dz, go = R.gate_backward(z, dx_out, ds_out, Ws, Wo, out_mul, skip_mul)
        assert (go is None) == (not with_dx)
        _close(dz, dz_t)
        dx, dc = R.data_backward(dz, go, Wd, Wa, dil, dc_accum)
        _close(dx, dx_t)
        _close(dc, dc_t)


def test_effective_weight_and_gate_saturation():
    w = torch.randn(4, 3, 2, generator=torch.Generator().manual_seed(0))
    s = torch.tensor([1.0, 2.0, -0.5, 0.0])
    assert torch.equal(R.effective(w), w.double())
    assert torch.equal(R.effective(w, s)[2], w[2].double() * -0.5) and R.effective(w, s).dtype == D
    z = torch.zeros(1, 128, 6, dtype=D)
    z[0, 0], z[0, 64] = torch.tensor([20.0, -20, 90, -90, 1e4, -1e4]), torch.tensor([1e4, 1e4, 90, 90, 20, -1e4])
    g = R.gate(z)[0, 0]
    assert torch.isfinite(g).all() and g.tolist()[:5] == pytest.approx([1, -1, 1, -1, 1], abs=1e-8) and g[5] == 0


# ------------------------------------------------------------------------------------------------ completeness
def _entry_points():
    src = open(os.path.join(ROOT, "parallelwavegan_amd", "csrc", "wavenet.hip")).read()
    block = src[src.index('extern "C" {'):]
    return re.findall(r"^(?:int|size_t) (pwg_wavenet_\w+)\(", block, re.M)


def test_every_entry_point_names_the_test_that_drives_it():
    names = _entry_points()
    assert len(names) == 10 and "pwg_wavenet_gate_backward" in names and "pwg_wavenet_layer_supported" in names, names
    gpu = importlib.import_module("tests.test_wavenet_matrix_gpu")
    missing = [n for n in names if n not in gpu.COVERED]
    assert not missing, f"entry points with no direct test: {missing}"
    stale = [n for n in gpu.COVERED if n not in names]
    assert not stale, f"COVERED names entry points that no longer exist: {stale}"
    module_marks = getattr(gpu, "pytestmark", [])
    module_marks = list(module_marks) if isinstance(module_marks, (list, tuple)) else [module_marks]
    for name, where in gpu.COVERED.items():
        if where.endswith(".py"):
            assert os.path.exists(os.path.join(ROOT, where)), f"{name}: {where} does not exist"
        else:
            fn = getattr(gpu, where, None)
            assert callable(fn) and where.startswith("test_"), f"{name}: no test function {where}"
            marks = module_marks + list(getattr(fn, "pytestmark", []))
            assert any(m.name == "gpu" for m in marks), f"{where} is not marked gpu"


# ------------------------------------------------------------------------------------------------ refusal table
# (kwargs of ops.make_wavenet_desc over the PWG.v1 defaults batch = 2, t = 100, dilation = 4) -> supported
GEOMETRIES = [
    (dict(t=1), True),
    (dict(batch=65535), True),
    (dict(aux_channels=79), False),
    (dict(aux_channels=72), False),
    (dict(aux_channels=88), False),
    (dict(causal=True), False),
    (dict(residual_channels=32), False),
    (dict(gate_channels=64), False),
    (dict(skip_channels=128), False),
    (dict(kernel=5), False),
    (dict(t=0), False),
    (dict(dilation=0), False),
    (dict(batch=0), False),
    (dict(batch=65536), False),
    (dict(t=2 ** 23), False),  # 128 * t * 4 reaches 2^32: past a 32-bit buffer range
    (dict(t=2 ** 23 - 1), True),
]


@pytest.mark.parametrize("kwargs,supported", GEOMETRIES, ids=[f"{k}" for k, _ in GEOMETRIES])
def test_supported_geometries_are_the_table(kwargs, supported):
    from parallelwavegan_amd import _lib, ops

    lib = _lib.lib()
    kw = dict(batch=2, t=100, dilation=4)
    kw.update(kwargs)
    d = ops.make_wavenet_desc(kw.pop("batch"), kw.pop("t"), kw.pop("dilation"), out_mul=math.sqrt(0.5), **kw)
    assert bool(lib.pwg_wavenet_layer_supported(ctypes.byref(d))) == supported
    sizes = [lib.pwg_wavenet_packed_weight_floats(ctypes.byref(d)), lib.pwg_wavenet_packed_weight_bwd_floats(ctypes.byref(d)),
             lib.pwg_wavenet_weight_backward_workspace_floats(ctypes.byref(d))]
    if supported:
        assert sizes[0] == 272 * 128 + 64 * 128 and sizes[1] == (16 * 2 + 48 * 2 + 16 * 3) * 256 and sizes[2] > 0, sizes
    else:
        assert sizes == [0, 0, 0], sizes
