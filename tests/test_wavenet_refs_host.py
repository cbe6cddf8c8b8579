"""CPU: the float64 references of tests/wavenet_refs.py against torch's own float64 evaluation and autograd of the
layer written tap by tap (so that the GPU matrix of tests/test_wavenet_matrix_gpu.py is compared with something that is
itself checked); the completeness check: every ``pwg_wavenet_*`` entry point of csrc/wavenet.hip must name, in
``COVERED``, the test that drives it directly; and the refusal table of ``pwg_wavenet_layer_supported``.

The weight path (tests/test_wavenet_wgrad_matrix_gpu.py): ``R.weight_backward`` and ``R.weight_norm_backward`` against
autograd, the slabs against their sum, the slicing plan (``pwg_wavenet_weight_backward_plan``, answered without a device)
at a table of shapes, and the room the data leave: over that module's grids the float32 CPU evaluation of the references
lies at most 7.0e-7 = 0.035 of its 2e-5 bar from float64 (about 29x of room), while a reference without one column, one tap or one slice lies more than
10 bars away at every row."""
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
    assert len(names) == 11 and "pwg_wavenet_gate_backward" in names and "pwg_wavenet_layer_supported" in names, names
    assert "pwg_wavenet_weight_backward" in names and "pwg_wavenet_weight_backward_plan" in names, names
    gpu = importlib.import_module("tests.test_wavenet_matrix_gpu")
    missing = [n for n in names if n not in gpu.COVERED]
    assert not missing, f"entry points with no direct test: {missing}"
    stale = [n for n in gpu.COVERED if n not in names]
    assert not stale, f"COVERED names entry points that no longer exist: {stale}"
    for name, where in gpu.COVERED.items():
        # ``test_name`` of the matrix itself, or ``module::test_name`` of another GPU module: a test function, never a file
        module, _, test = where.rpartition("::")
        mod = importlib.import_module(module) if module else gpu
        assert os.path.basename(mod.__file__).startswith("test_"), f"{name}: {module} is not a test module"
        fn = getattr(mod, test, None)
        assert callable(fn) and test.startswith("test_"), f"{name}: no test function {where}"
        module_marks = getattr(mod, "pytestmark", [])
        module_marks = list(module_marks) if isinstance(module_marks, (list, tuple)) else [module_marks]
        marks = module_marks + list(getattr(fn, "pytestmark", []))
        assert any(m.name == "gpu" for m in marks), f"{where} is not marked gpu"
    weight_path = [n for n in names if "weight_backward" in n]
    assert len(weight_path) == 3 and all(gpu.COVERED[n].startswith("tests.test_wavenet_wgrad_matrix_gpu::") for n in weight_path)


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


# ------------------------------------------------------------------------------------------------ the weight path
def _wgrad():
    return importlib.import_module("tests.test_wavenet_wgrad_matrix_gpu")


@pytest.mark.parametrize("with_go", [True, False])
@pytest.mark.parametrize("dil", [1, 3, 64])
@pytest.mark.parametrize("T", [1, 5, 33, 100])
def test_weight_backward_matches_torch_autograd(T, dil, with_go):
    """``R.weight_backward`` on ``dz``, ``gs = skip_mul * ds_out`` and ``go`` of ``R.gate_backward`` and the saved ``g``
    against autograd of the whole layer with respect to its four weights and three biases."""
    gen = torch.Generator().manual_seed(77 * T + dil)
    r = lambda *s: torch.randn(*s, dtype=D, generator=gen)  # noqa: E731
    B = 3
    x, c, ds_out, dx_out = r(B, 64, T), r(B, AUX, T), r(B, 64, T), r(B, 64, T)
    out_mul, skip_mul = math.sqrt(0.5), math.sqrt(1 / 30)
    leaves = [t.requires_grad_() for t in (r(128, 64, 3) / math.sqrt(192), r(128, AUX, 1) / math.sqrt(AUX), r(64, 64, 1) / 8,
                                           r(64, 64, 1) / 8, r(128), r(64), r(64))]
    Wd, Wa, Ws, Wo, b_d, b_s, b_o = leaves
    z, g, so, xo = R.layer_forward(x, c, None, Wd, Wa, Ws, Wo, b_d, b_s, b_o, dil, out_mul, skip_mul)
    loss = (so * ds_out).sum() + ((xo * dx_out).sum() if with_go else 0.0)
    want = torch.autograd.grad(loss, leaves, allow_unused=True)
    with torch.no_grad():
        dz, go = R.gate_backward(z, dx_out if with_go else None, ds_out, Ws, Wo, out_mul, skip_mul)
        got = R.weight_backward(dz, x, c, skip_mul * ds_out, go, g, dil)
    assert (got["dWo"] is None) == (got["db_out"] is None) == (not with_go)
    for k, ref in zip(("dWd", "dWa", "dWs", "dWo", "db_dil", "db_skip", "db_out"), want):
        if got[k] is None:
            assert ref is None, k
        else:
            _close(got[k], ref)


def test_weight_norm_backward_matches_torch_autograd():
    gen = torch.Generator().manual_seed(3)
    for shape in ((128, 64, 3), (128, AUX, 1), (64, 64, 1), (5, 1, 1)):
        v = torch.randn(shape, dtype=D, generator=gen).requires_grad_()
        g = (0.5 + torch.rand(shape[0], dtype=D, generator=gen)).requires_grad_()
        dw = torch.randn(shape, dtype=D, generator=gen)
        w = g.view(-1, 1, 1) * v / v.flatten(1).norm(dim=1).view(-1, 1, 1)
        dv_t, dg_t = torch.autograd.grad((w * dw).sum(), (v, g))
        dv, dg = R.weight_norm_backward(dw, v.detach(), g.detach())
        _close(dv, dv_t)
        _close(dg, dg_t)
        assert R.weight_norm_backward(dw, v.detach(), g.detach().view(-1, 1, 1))[1].shape == (shape[0], 1, 1)


# (B, T, chunks per slice of the two launches): runs that straddle items, that end on a single chunk, one chunk in total
SLAB_PLANS = [(5, 7, (2, 2)), (3, 96, (2, 3)), (3, 95, (2, 2)), (4, 200, (3, 7)), (1, 20, (1, 1)), (2, 131, (2, 2))]


@pytest.mark.parametrize("B,T,per", SLAB_PLANS)
@pytest.mark.parametrize("with_go", [True, False])
def test_slabs_sum_to_the_weight_gradients(B, T, per, with_go):
    gen = torch.Generator().manual_seed(B * 1000 + T)
    dil = 3
    dz, x, c, gs, go, g = [torch.randn(B, ch, T, dtype=D, generator=gen) for ch in (128, 64, AUX, 64, 64, 64)]
    go = go if with_go else None
    for p in set(per):
        ranges = R.slab_ranges(B, T, p)
        owned = sorted((b, n) for rs in ranges for b, lo, hi in rs for n in range(lo, hi))
        assert owned == [(b, n) for b in range(B) for n in range(T)], "every column in exactly one slice"
        assert len(ranges) == -(-(B * -(-T // 32)) // p)
        assert all(lo % 32 == 0 and (hi % 32 == 0 or hi == T) for rs in ranges for _, lo, hi in rs)
    if (B, T) != (1, 20):
        assert any(len(rs) > 1 for rs in R.slab_ranges(B, T, per[0])), "the plan straddles two items"
    s0, s1 = R.weight_backward_slabs(dz, x, c, gs, go, g, dil, per)
    assert s0.shape == (len(R.slab_ranges(B, T, per[0])), 128, 273) and s1.shape == (len(R.slab_ranges(B, T, per[1])), 128, 65)
    ref = R.weight_backward(dz, x, c, gs, go, g, dil)
    t0, t1 = s0.sum(0), s1.sum(0)
    _close(t0[:, :192].view(128, 3, 64).permute(0, 2, 1), ref["dWd"])  # columns [tap0 x | tap1 x | tap2 x | c | row sum]
    _close(t0[:, 192:272, None], ref["dWa"])
    _close(t0[:, 272], ref["db_dil"])
    _close(t1[:64, :64, None], ref["dWs"])
    _close(t1[:64, 64], ref["db_skip"])
    if with_go:
        _close(t1[64:, :64, None], ref["dWo"])
        _close(t1[64:, 64], ref["db_out"])
    else:
        assert float(t1[64:].abs().max()) == 0.0


# (B, T) -> (slices0, chunks per slice 0, slices1, chunks per slice 1): one chunk in total; one chunk per item; a
# straddling plan; at most 2 chunks per slice up to 512 (resp. 1536) chunks, 3 from the first count above it
PLANS = [
    ((1, 1), (1, 1, 1, 1)),
    ((1, 32), (1, 1, 1, 1)),
    ((1, 33), (1, 2, 1, 2)),
    ((5, 7), (3, 2, 3, 2)),
    ((5, 32), (3, 2, 3, 2)),
    ((3, 95), (5, 2, 5, 2)),
    ((1, 32 * 512), (256, 2, 256, 2)),
    ((1, 32 * 512 + 1), (171, 3, 257, 2)),
    ((27, 19 * 32), (171, 3, 257, 2)),
    ((1, 32 * 1536), (256, 6, 768, 2)),
    ((1, 32 * 1536 + 1), (220, 7, 513, 3)),
    ((3, 5500), (172, 3, 258, 2)),
    ((7, 7100), (222, 7, 518, 3)),
    ((6, 25600), (253, 19, 686, 7)),  # ceil(4800 / 256) = 19, ceil(4800 / 768) = 7
]


@pytest.mark.parametrize("shape,plan", PLANS, ids=[f"B{b}-T{t}" for (b, t), _ in PLANS])
def test_weight_backward_plan_is_the_table(shape, plan):
    from parallelwavegan_amd import _lib, ops

    lib = _lib.lib()
    for dil in (1, 512):
        d = ops.make_wavenet_desc(*shape, dil)
        out = (ctypes.c_int32 * 4)()
        assert lib.pwg_wavenet_weight_backward_plan(ctypes.byref(d), out) == 0
        assert tuple(out) == plan
        assert ops.wavenet_weight_backward_plan(d) == dict(slices=(plan[0], plan[2]), chunks_per_slice=(plan[1], plan[3]))
        assert lib.pwg_wavenet_weight_backward_workspace_floats(ctypes.byref(d)) == plan[0] * 128 * 273 + plan[2] * 128 * 65
        for i in (0, 2):  # the slices are the runs of R.slab_ranges
            assert len(R.slab_ranges(*shape, plan[i + 1])) == plan[i]


def test_weight_backward_plan_refusals():
    from parallelwavegan_amd import _lib, ops

    lib = _lib.lib()
    out = (ctypes.c_int32 * 4)(*[-7] * 4)
    assert lib.pwg_wavenet_weight_backward_plan(ctypes.byref(ops.make_wavenet_desc(2, 35, 3)), None) == -4  # PWG_ERR_NULL
    assert b"NULL out" in lib.pwg_last_error()
    for bad in (ops.make_wavenet_desc(2, 35, 3, causal=True), ops.make_wavenet_desc(2, 35, 3, aux_channels=72), None):
        assert lib.pwg_wavenet_weight_backward_plan(None if bad is None else ctypes.byref(bad), out) == -2  # PWG_ERR_UNSUPPORTED
        assert b"unsupported layer geometry" in lib.pwg_last_error()
    assert list(out) == [-7] * 4
    with pytest.raises(RuntimeError, match="unsupported layer geometry"):
        ops.wavenet_weight_backward_plan(ops.make_wavenet_desc(2, 35, 3, kernel=5))


def _rel(a, b):
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-12)


def test_float32_room_and_sensitivity():
    """Over the GPU grids (a) and (c) of tests/test_wavenet_wgrad_matrix_gpu.py, on that module's own operands: the
    float32 CPU evaluation of the references (final gradients and slabs) against float64, relative to the bar -- the room
    the data leave -- and what the bar resolves: a reference without one column, one tap or one slice lies more than 10
    bars away at every row."""
    W = _wgrad()
    rows = [(2, T, dil) for T, dil in W.EDGE_GRID] + list(W.SLICING_GRID)
    worst = 0.0
    for B, T, dil in rows:
        ops64 = W._f64(B, T)
        ref = R.weight_backward(*ops64, dil)
        chunks = B * -(-T // 32)
        per = (2, 2) if chunks >= 2 else (1, 1)
        slabs = R.weight_backward_slabs(*ops64, dil, per)
        ops32 = [W._data(B, T)[n] for n in W.OPERANDS]
        f32 = R.weight_backward(*ops32, dil)
        assert all(v.dtype == torch.float32 for v in f32.values())
        errs = [_rel(f32[k].double(), ref[k]) for k in ref]
        errs += [_rel(a.double(), b) for a, b in zip(R.weight_backward_slabs(*ops32, dil, per), slabs)]
        worst = max(worst, max(errs))
        # one column less: the last column of the last item, in both 128-row operands
        cut = [t.clone() for t in ops64]
        for i in (0, 3, 4):
            cut[i][B - 1, :, T - 1] = 0
        moved = R.weight_backward(*cut, dil)
        for k in ref:
            assert _rel(moved[k], ref[k]) > 10 * W.RTOL, (B, T, dil, k)
        # one tap less (a tap that lies wholly outside the sequence, dil >= T, contributes nothing to begin with)
        for k in range(3):
            if k == 1 or dil < T:
                assert ref["dWd"][:, :, k].abs().max().item() / ref["dWd"].abs().max().item() > 10 * W.RTOL, (B, T, dil, k)
            else:
                assert float(ref["dWd"][:, :, k].abs().max()) == 0.0
        # one slice less
        for s in slabs:
            for drop in {0, s.shape[0] - 1}:
                assert _rel(s.sum(0) - s[drop], s.sum(0)) > 10 * W.RTOL, (B, T, dil, drop)
    print(f"float32 CPU evaluation: worst rel-to-max distance from float64 {worst:.3e} = {worst / W.RTOL:.4f} of the bar")
    assert worst <= W.RTOL / 10, worst
