"""CPU: what makes tests/optim_refs.py trustworthy, and the host-side assumptions of optimizers/fused.py.

* ``hyper="exact"`` in float64 IS torch.optim.Adam / AdamW (non-fused) and the restated RAdam of oracle/radam.py;
* the float32 evaluation of every reference lies inside the reference's own bound (the worst ratio is printed: above 1
  the count of roundings is wrong, not the data);
* ``"as_passed"`` and ``"exact"`` differ by no more than ``mode_distance_bound`` says;
* ``_chunk_for``, the 48-byte chunk record, and the state-dict interchange with torch.optim.Adam, without a launch.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import radam as oracle_radam
from parallelwavegan_amd.optimizers import fused
from tests import optim_refs as R
from tests.elementwise_refs import U

D = torch.float64
F = torch.float32
N = 70000  # one tensor of the GPU test's largest size

# (kind, keyword arguments) the GPU matrix draws from; every one at every t below
CONFIGS = [
    ("adam", dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0), False),
    ("adam", dict(lr=2e-4, betas=(0.5, 0.9), eps=1e-6, weight_decay=0.01, grad_scale=0.5), True),
    ("adam", dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, grad_scale=1.0), True),
    ("adamw", dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, grad_scale=0.5), False),
    ("adamw", dict(lr=2e-4, betas=(0.5, 0.9), eps=1e-6, weight_decay=0.0, grad_scale=1.0), True),
    ("radam", dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0), False),
    ("radam", dict(lr=2e-4, betas=(0.5, 0.9), eps=1e-6, weight_decay=0.01, grad_scale=0.5), False),
    ("radam", dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=-0.01, grad_scale=0.5), False),
]
STEPS = (1, 5, 6, 1000, 10 ** 6)


def _call(kind, fam, dtype, amsgrad, t, hyper, entry, kw):
    return R.step(kind, fam, dtype, amsgrad, t, hyper, entry, **kw)


def _ratios(got, ref):
    out = {}
    for name, b in (("p", "bp"), ("m", "bm"), ("v", "bv"), ("vmax", "bvmax")):
        if getattr(ref, name) is not None:
            out[name] = R.ratio(getattr(got, name), getattr(ref, name), getattr(ref, b))
    return out


# ------------------------------------------------------------------------------------------------- against torch
def _close(a, b, what):
    a, b = a.detach().to(D), b.detach().to(D)
    assert (a - b).abs().max().item() <= 1e-12 * max(b.abs().max().item(), 1e-300), what


@pytest.mark.parametrize("cls,kw", [
    (torch.optim.Adam, dict(lr=1e-3)),
    (torch.optim.Adam, dict(lr=1e-3, weight_decay=0.01)),
    (torch.optim.Adam, dict(lr=1e-3, eps=1e-6, amsgrad=True)),
    (torch.optim.Adam, dict(lr=2e-4, betas=(0.5, 0.9), weight_decay=0.01, amsgrad=True)),
    (torch.optim.AdamW, dict(lr=1e-3)),  # torch's default decay 1e-2
    (torch.optim.AdamW, dict(lr=1e-3, weight_decay=0.05, amsgrad=True)),
    (torch.optim.AdamW, dict(lr=2e-4, betas=(0.5, 0.9), weight_decay=0.0)),
])
def test_exact_float64_is_torch(cls, kw):
    gen = torch.Generator().manual_seed(11)
    pt = torch.randn(257, generator=gen, dtype=D).requires_grad_()
    opt = cls([pt], foreach=False, **kw)
    grp = opt.param_groups[0]
    p = pt.detach().clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    vmax = torch.zeros_like(p) if grp["amsgrad"] else None
    for t in range(1, 9):
        g = torch.randn(257, generator=gen, dtype=D) * (10.0 if t == 3 else 0.1)
        pt.grad = g.clone()
        opt.step()
        r = R.adam_step(p, g, m, v, vmax, lr=grp["lr"], betas=grp["betas"], eps=grp["eps"],
                        weight_decay=grp["weight_decay"], t=t, decoupled=cls is torch.optim.AdamW, hyper="exact")
        p, m, v, vmax = r.p, r.m, r.v, r.vmax
        st = opt.state[pt]
        assert int(st["step"]) == t
        _close(p, pt, f"p at step {t}")
        _close(m, st["exp_avg"], f"exp_avg at step {t}")
        _close(v, st["exp_avg_sq"], f"exp_avg_sq at step {t}")
        if vmax is not None:
            _close(vmax, st["max_exp_avg_sq"], f"max_exp_avg_sq at step {t}")


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.9, 0.99), (0.5, 0.9), (0.5, 0.5)])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_exact_float64_is_the_restated_radam(betas, wd):
    gen = torch.Generator().manual_seed(12)
    po = torch.randn(257, generator=gen, dtype=D)
    mo, vo = torch.zeros_like(po), torch.zeros_like(po)
    p, m, v = po.clone(), mo.clone(), vo.clone()
    for t in range(1, 9):
        g = torch.randn(257, generator=gen, dtype=D)
        oracle_radam.radam_step(po, g, mo, vo, t, lr=1e-3, betas=betas, eps=1e-6, weight_decay=wd)
        r = R.radam_step(p, g, m, v, lr=1e-3, betas=betas, eps=1e-6, weight_decay=wd, t=t, hyper="exact")
        p, m, v = r.p, r.m, r.v
        _close(p, po, f"p at step {t}")
        _close(m, mo, f"exp_avg at step {t}")
        _close(v, vo, f"exp_avg_sq at step {t}")
        # the rectified branch starts at step 6 for 0.999 / 0.99 / 0.9 and never for 0.5 (N_max = 3 < 5)
        for hyper, entry in (("exact", "dev"), ("as_passed", "dev"), ("as_passed", "host")):
            assert R.radam_scalars(1e-3, betas, t, hyper, entry)[1] == (betas[1] != 0.5 and t >= 6)
    if betas[1] == 0.5:
        assert 2.0 / (1.0 - betas[1]) - 1.0 == 3.0
        assert not any(R.radam_scalars(1e-3, betas, t, "exact")[1] for t in (10, 100, 1000, 10 ** 6))


# ------------------------------------------------------------------------------------------------- own bounds
WORST = {}


@pytest.mark.parametrize("entry", ["dev", "host"])
@pytest.mark.parametrize("t", STEPS)
@pytest.mark.parametrize("ci", range(len(CONFIGS)))
def test_float32_evaluation_is_inside_the_bounds(ci, t, entry):
    kind, kw, amsgrad = CONFIGS[ci]
    if kind == "adamw":
        kw = dict(kw, weight_decay=abs(kw["weight_decay"]))
    fam = R.family(N, t, seed=ci)
    ref = _call(kind, fam, D, amsgrad, t, "as_passed", entry, kw)
    got = _call(kind, fam, F, amsgrad, t, "as_passed", entry, kw)
    rs = _ratios(got, ref)
    for k, r in rs.items():
        WORST[(kind, k)] = max(WORST.get((kind, k), 0.0), r)
    print(f"{kind} t={t} {entry}: float32 / bound " + " ".join(f"{k}={r:.3f}" for k, r in rs.items()))
    assert all(r <= 1.0 for r in rs.values()), rs


@pytest.mark.parametrize("sizes,scale,max_norm", [
    ((1, 255, 65535, 65536, 65537, 140000), 1.0, 10.0),
    ((1, 255, 65535, 65536, 65537, 140000), 1.0, 1e4),
    ((3,), 1e-3, 1.0),
])
def test_float32_clip_is_inside_the_bounds(sizes, scale, max_norm):
    gs = [R.family(n, 2, seed=40 + i).g * scale for i, n in enumerate(sizes)]
    ref = R.clip([g.to(D) for g in gs], max_norm)
    got = R.clip(gs, max_norm)
    rs = dict(norm=R.ratio(got.norm, ref.norm, ref.bnorm), coef=R.ratio(got.coef, ref.coef, ref.bcoef),
              grads=max(R.ratio(a, b, c) for a, b, c in zip(got.grads, ref.grads, ref.bgrads)))
    print("clip: float32 / bound " + " ".join(f"{k}={r:.3f}" for k, r in rs.items()))
    assert all(r <= 1.0 for r in rs.values()), rs
    # and float64 is torch.nn.utils.clip_grad_norm_
    ps = [torch.nn.Parameter(torch.zeros_like(g, dtype=D)) for g in gs]
    for p, g in zip(ps, gs):
        p.grad = g.to(D).clone()
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    assert abs(float(total) - float(ref.norm)) <= 1e-12 * float(ref.norm)
    for p, g in zip(ps, ref.grads):
        assert (p.grad - g).abs().max().item() <= 1e-12 * g.abs().max().item()


def test_worst_ratios_are_printed():
    """Runs after the parametrised cases of this module: the summary line the issue asks for."""
    print("worst float32 / bound: " + ", ".join(f"{k[0]}.{k[1]}={r:.3f}" for k, r in sorted(WORST.items())))
    assert all(r <= 1.0 for r in WORST.values())


# ------------------------------------------------------------------------------------------------- mode distance
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9), (0.8, 0.99)])
@pytest.mark.parametrize("t", STEPS)
@pytest.mark.parametrize("kind,wd,amsgrad", [("adam", 0.01, True), ("adam", 0.0, False), ("adamw", 0.01, False),
                                             ("radam", 0.01, False)])
def test_modes_differ_by_the_derived_bound(kind, wd, amsgrad, t, betas):
    """``as_passed`` - ``exact`` in float64.  The moments: the factor ``1 - b`` moves by ``d = U / (1 - b)`` relative,
    everything else by ``U``, which the rounding bound of the same output already holds.  ``p'``: the update is
    ``step_size m' / d(v')``; ``step_size`` moves by ``d1`` (``t b^t / (1 - b^t) <= b / (1 - b)``; RAdam:
    ``radam_step_size_distance``), ``m'`` by ``d1 S_m``, ``v'`` by ``d2 v'`` and ``sqrt(1 - b2^t)`` by ``d2 / 2``, so
    the denominator is no smaller than ``d_lo`` below; second-order terms double the first-order ones."""
    kw = dict(lr=1e-3, betas=betas, eps=1e-8, weight_decay=wd, grad_scale=0.5)
    fam = R.family(N, t, seed=7)
    a = _call(kind, fam, D, amsgrad, t, "as_passed", "dev", kw)
    e = _call(kind, fam, D, amsgrad, t, "exact", "dev", kw)
    d1, d2 = R.mode_distance_bound(*betas)
    g = fam.g.to(D) * 0.5
    s_g = g.abs() + (abs(wd * fam.p.to(D)) if kind == "adam" else 0)
    s_m = betas[0] * fam.m.to(D).abs() + (1 - betas[0]) * s_g
    s_v = betas[1] * fam.v.to(D) + (1 - betas[1]) * s_g * s_g
    dm, dv = d1 * (1 - betas[0]) * s_g + a.bm, d2 * (1 - betas[1]) * s_g * s_g + a.bv
    assert bool(((a.m - e.m).abs() <= dm).all())
    assert bool(((a.v - e.v).abs() <= dv).all())
    print(f"{kind} {betas} t={t}: measured relative distance of v' "
          f"{((a.v - e.v).abs() / e.v.clamp(min=1e-300)).max().item():.3e}, bound {d2:.3e}")
    vv = e.v if e.vmax is None else e.vmax
    if kind == "radam":
        step, rect = R.radam_scalars(1e-3, betas, t, "exact")
        aux, dstep = 1.0, R.radam_step_size_distance(betas, t)
    else:
        num, div, aux, _ = R.adam_scalars(1e-3, betas, t, "exact")
        step, rect, dstep = num / div, True, 2 * (d1 + 2 * U)
    if rect:
        d = torch.sqrt(vv) / aux + 1e-8
        d_lo = (torch.sqrt(torch.clamp(vv - dv, min=0)) / aux + 1e-8) * (1 - d2 - 4 * U)
        dp = a.bp + step * e.m.abs() * (1 / d_lo - 1 / d) + (dstep + 2 * d1) * step * s_m / d_lo
    else:
        dp = a.bp + (dstep + 2 * d1) * step * s_m
    assert bool(((a.p - e.p).abs() <= dp).all()), ((a.p - e.p).abs() / dp).max().item()
    if betas[1] == 0.999 and t == 1 and kind == "adam" and not wd:
        # the figure of the module docstring: exp_avg_sq of the first step is (1 - b2) g^2
        nz = e.v > 0
        rel = ((a.v[nz] - e.v[nz]).abs() / e.v[nz]).max().item()
        assert 1.28e-5 < rel < 1.30e-5 and rel <= d2


# ------------------------------------------------------------------------------------------------- host assumptions
def test_chunk_sizes():
    mi = 1 << 20
    assert fused.CHUNK == R.CLIP_CHUNK == 65536
    assert [fused._chunk_for(n) for n in (1, 78869, 8 * mi)] == [4096, 4096, 4096]
    assert fused._chunk_for(8 * mi + 1) == 8192
    assert fused._chunk_for(16 * mi) == 8192
    assert fused._chunk_for(16 * mi + 1) == 16384
    assert fused._chunk_for(128 * mi) == 65536
    assert fused._chunk_for(10 ** 9) == 65536


class OptChunk(ctypes.Structure):
    """``pwg_opt_chunk`` of include/pwg_kernels.h."""
    _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_void_p), ("m", ctypes.c_void_p), ("v", ctypes.c_void_p),
                ("vmax", ctypes.c_void_p), ("n", ctypes.c_int32), ("pad_", ctypes.c_int32)]


def test_chunk_record_is_one_row_of_six_int64():
    assert ctypes.sizeof(OptChunk) == 48
    row = (0x7F0012345670, 0x7F00ABCDEF04, 0x7F0000000010, 0x7F00FFFFFFF0, 0, 65536)
    rec = OptChunk(*row[:5], row[5], 0)
    assert bytes(rec) == np.asarray([row], dtype=np.int64).tobytes()
    assert OptChunk.n.offset == 40 and OptChunk.vmax.offset == 32


def test_every_optimizer_entry_point_names_its_direct_test():
    import importlib
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "pwg_kernels.h")).read()
    names = set(re.findall(r"\bint\s+(pwg_(?:r?adam_step\w*|clip_grad_norm))\s*\(", header))
    assert len(names) == 5
    gpu = importlib.import_module("tests.test_optim_matrix_gpu")
    assert set(gpu.COVERED) == names
    for name, where in gpu.COVERED.items():
        assert callable(getattr(gpu, where, None)), f"{name}: no test {where}"


def test_state_dict_interchange_with_torch_adam():
    """Both directions on the CPU, nothing launched: torch's tensor ``step`` loads into the fused class, the fused
    class's int ``step`` loads into torch.optim.Adam, which then takes the next step from it."""
    gen = torch.Generator().manual_seed(5)
    kw = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, amsgrad=True)
    pt = [torch.randn(n, generator=gen, dtype=D).requires_grad_() for n in (7, 33)]
    ref = torch.optim.Adam(pt, foreach=False, **kw)
    for _ in range(2):
        for p in pt:
            p.grad = torch.randn(p.shape, generator=gen, dtype=D)
        ref.step()
    sd = ref.state_dict()
    assert isinstance(sd["state"][0]["step"], torch.Tensor)
    pf = [p.detach().clone().requires_grad_() for p in pt]
    opt = fused.Adam(pf, **kw)
    opt.load_state_dict(sd)
    for a, b in zip(pf, pt):
        st, sr = opt.state[a], ref.state[b]
        assert set(st) == set(sr) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}
        assert opt._as_int(st["step"]) == 2
        for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
            assert torch.equal(st[k], sr[k])
    # the other way: a state as the fused class keeps it (int step), written without a launch
    for i, a in enumerate(pf):
        st = opt.state[a]
        st["step"] = 3
        fam = R.family(a.numel(), 4, seed=60 + i)
        st["exp_avg"], st["exp_avg_sq"] = fam.m.to(D), fam.v.to(D)
        st["max_exp_avg_sq"] = fam.vmax.to(D)
    sd = opt.state_dict()
    assert all(type(s["step"]) is int for s in sd["state"].values())
    pb = [a.detach().clone().requires_grad_() for a in pf]
    back = torch.optim.Adam(pb, foreach=False, **kw)
    back.load_state_dict(sd)
    want = []
    for a, b in zip(pf, pb):
        b.grad = torch.randn(b.shape, generator=gen, dtype=D)
        st = opt.state[a]
        want.append(R.adam_step(a.detach(), b.grad, st["exp_avg"], st["exp_avg_sq"], st["max_exp_avg_sq"],
                                lr=kw["lr"], betas=kw["betas"], eps=kw["eps"], weight_decay=kw["weight_decay"], t=4,
                                hyper="exact"))
    back.step()
    for b, r in zip(pb, want):
        assert int(back.state[b]["step"]) == 4
        _close(b, r.p, "p after the step from the loaded state")
        _close(back.state[b]["exp_avg"], r.m, "exp_avg")
        _close(back.state[b]["exp_avg_sq"], r.v, "exp_avg_sq")
        _close(back.state[b]["max_exp_avg_sq"], r.vmax, "max_exp_avg_sq")
