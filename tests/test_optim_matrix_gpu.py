"""GPU: the optimizer and gradient-clipping kernels of csrc/reduce_optim.hip (``adam_multi[_dev]_kernel``,
``radam_multi[_dev]_kernel``, ``sqsum_multi_kernel``, ``clip_coef_kernel``, ``scale_grads_multi_kernel``) and the host
code that feeds them (optimizers/fused.py), ONE STEP AT A TIME from a given state against the float64 references of
tests/optim_refs.py (``hyper="as_passed"``: the scalars as the kernels receive them).

Every output of a step -- ``p'``, ``exp_avg``, ``exp_avg_sq``, ``max_exp_avg_sq`` -- lies within the reference's own
bound (sums of absolute values of terms times a counted number of roundings; tests/test_optim_refs_host.py shows that
a float32 CPU evaluation stays inside them), the step count advances, the gradient is bit-unchanged.  What is exact is
compared bit for bit: the cut into chunks, a captured step against an eager twin, the clip coefficient computed from the
kernel's own norm, the scaled gradients, memory outside the slices.  Each comparison prints ``<output>: err / bound``.
"""
import math

import numpy as np
import pytest
import torch

from parallelwavegan_amd import _lib, optimizers
from parallelwavegan_amd.ops import _stream
from parallelwavegan_amd.optimizers import fused
from tests import optim_refs as R
from tests.util import poison_empty

pytestmark = pytest.mark.gpu

D = torch.float64
GUARD = 64             # floats of guard band on each side of a slice      } as in tests/test_conv_cfg_matrix_gpu.py
SENTINEL = 0x7FC5A5A5  # a quiet NaN with a payload no kernel produces     }
SIZES = (1, 3, 255, 256, 257, 4096, 4097, 70000)  # one group: 78 869 elements, 4096-element chunks
CLASSES = {"adam": optimizers.Adam, "adamw": optimizers.AdamW, "radam": optimizers.RAdam}
A, B = (0.9, 0.999), (0.5, 0.9)
# optimizer entry point of include/pwg_kernels.h -> the test below that drives it directly
COVERED = {
    "pwg_adam_step": "test_host_scalar_entry_points",
    "pwg_radam_step": "test_host_scalar_entry_points",
    "pwg_adam_step_dev": "test_dev_entry_points_on_a_mixed_table",
    "pwg_radam_step_dev": "test_dev_entry_points_on_a_mixed_table",
    "pwg_clip_grad_norm": "test_clip_grad_norm",
}
WORST = {}  # output -> largest err / bound seen on the GPU (printed by the last test of the module)


def _within(what, got, ref, bound, key):
    r = R.ratio(got, ref, bound)
    WORST[key] = max(WORST.get(key, 0.0), r)
    print(f"{what}: {key} err / bound = {r:.3f}")
    assert r <= 1.0, f"{what}: {key} is {r:.3f} times its bound away from the float64 reference"


def _check_step(what, got, ref):
    """``got``: (p, exp_avg, exp_avg_sq, max_exp_avg_sq or None) after the step; ``ref``: the reference's ``Step``."""
    for name, val, want, bound in (("p", got[0], ref.p, ref.bp), ("m", got[1], ref.m, ref.bm),
                                   ("v", got[2], ref.v, ref.bv), ("vmax", got[3], ref.vmax, ref.bvmax)):
        assert (val is None) == (want is None), f"{what}: {name}"
        if want is not None:
            _within(what, val, want, bound, name)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _inject(opt, p, fam, t, amsgrad):
    st = opt.state[p]
    st["step"] = t - 1
    st["exp_avg"], st["exp_avg_sq"] = fam.m.to(p.device), fam.v.to(p.device)
    if amsgrad:
        st["max_exp_avg_sq"] = fam.vmax.to(p.device)


def _optimizer(device, kind, sizes, t, kw, amsgrad=False, grad_scale=1.0, seed=0):
    amsgrad = amsgrad and kind != "radam"
    fams = [R.family(n, t, seed + i) for i, n in enumerate(sizes)]
    params = [f.p.clone().to(device).requires_grad_() for f in fams]
    opt = CLASSES[kind](params, **(kw if kind == "radam" else dict(kw, amsgrad=amsgrad)))
    opt.grad_scale = grad_scale
    for p, f in zip(params, fams):
        p.grad = f.g.to(device)
        _inject(opt, p, f, t, amsgrad)
    return opt, params, fams


def _state(opt, p):
    st = opt.state[p]
    return p.detach(), st["exp_avg"], st["exp_avg_sq"], st.get("max_exp_avg_sq")


def _snapshot(opt, p, g):
    """The state on the device before a step, as a ``Family`` of CPU tensors."""
    _, m, v, vmax = _state(opt, p)
    return R.Family(p.detach().cpu().clone(), g.detach().cpu().clone(), m.cpu().clone(), v.cpu().clone(),
                    None if vmax is None else vmax.cpu().clone())


# ------------------------------------------------------------------------------------------ through the classes
# t, betas, weight_decay, amsgrad, grad_scale, eps, lr: every value of every factor with every class
ROWS = [
    (1, A, 0.0, False, 1.0, 1e-8, 1e-3),
    (1, B, 0.01, True, 0.5, 1e-6, 2e-4),
    (2, B, 0.01, True, 0.5, 1e-6, 1e-3),
    (5, A, 0.01, True, 1.0, 1e-6, 1e-3),
    (5, B, 0.0, False, 0.5, 1e-8, 2e-4),
    (6, A, 0.0, False, 0.5, 1e-8, 1e-3),
    (6, B, 0.01, True, 1.0, 1e-6, 2e-4),
    (6, A, 0.01, False, 1.0, 1e-8, 1e-3),
    (1000, B, 0.0, True, 1.0, 1e-8, 1e-3),
    (1000, A, 0.01, False, 0.5, 1e-6, 2e-4),
    (10 ** 6, A, 0.01, False, 0.5, 1e-6, 1e-3),
    (10 ** 6, B, 0.0, True, 1.0, 1e-8, 2e-4),
]


@pytest.mark.parametrize("row", ROWS, ids=lambda r: f"t{r[0]}-b{r[1][1]}-wd{r[2]}-ams{int(r[3])}-s{r[4]}-eps{r[5]}")
@pytest.mark.parametrize("kind", ["adam", "adamw", "radam"])
def test_one_step_through_the_class(kind, row, device):
    t, betas, wd, amsgrad, grad_scale, eps, lr = row
    amsgrad = amsgrad and kind != "radam"
    kw = dict(lr=lr, betas=betas, eps=eps, weight_decay=wd)
    opt, params, fams = _optimizer(device, kind, SIZES, t, kw, amsgrad, grad_scale, seed=t % 97)
    assert fused._chunk_for(sum(SIZES)) == 4096
    if kind == "radam" and betas == A:
        assert opt._hyper(opt.param_groups[0], t)[6] == (1.0 if t >= 6 else 0.0)  # t = 5 | 6: both branches
    opt.step()
    torch.cuda.synchronize()
    assert opt._dev[0]["n_chunks"] == sum(-(-n // 4096) for n in SIZES)
    for p, f in zip(params, fams):
        ref = R.step(kind, f, D, amsgrad, t, grad_scale=grad_scale, **kw)
        _check_step(f"{kind} t={t} n={p.numel()}", _state(opt, p), ref)
        assert opt.state[p]["step"] == t
        assert _same_bits(p.grad, f.g), "the gradient was written"


@pytest.mark.parametrize("kind", ["adam", "radam"])
def test_the_cut_into_chunks_does_not_change_a_bit(kind, device, monkeypatch):
    """``_chunk_for``: "element-wise updates do not depend on the cut".  8192 and 65536 are what real models get (the
    latter cuts the 70000-element tensor into 65536 + 4464); the test group alone would only ever see 4096."""
    sizes = (70000, 257, 4097)
    kw = dict(lr=1e-3, betas=A, eps=1e-8, weight_decay=0.01)
    runs = {}
    for chunk in (4096, 8192, 65536):
        monkeypatch.setattr(fused, "_chunk_for", lambda total, c=chunk: c)
        opt, params, fams = _optimizer(device, kind, sizes, 6, kw, amsgrad=True, grad_scale=0.5, seed=3)
        opt.step()
        torch.cuda.synchronize()
        assert opt._dev[0]["n_chunks"] == sum(-(-n // chunk) for n in sizes)
        runs[chunk] = [[None if x is None else x.cpu().clone() for x in _state(opt, p)] for p in params]
    for p, f, got in zip(params, fams, runs[4096]):
        _check_step(f"{kind} chunk 4096 n={p.numel()}", got, R.step(kind, f, D, True, 6, grad_scale=0.5, **kw))
    for chunk in (8192, 65536):
        for a, b in zip(runs[4096], runs[chunk]):
            for x, y in zip(a, b):
                assert (x is None and y is None) or _same_bits(x, y), f"chunk {chunk} differs from chunk 4096"


# ------------------------------------------------------------------------------------------ bookkeeping
def test_two_groups_with_their_own_lr_and_decay(device):
    fams = [R.family(n, 5, 20 + i) for i, n in enumerate((257, 4097, 70000))]
    params = [f.p.clone().to(device).requires_grad_() for f in fams]
    kws = [dict(lr=1e-3, weight_decay=0.0), dict(lr=3e-4, weight_decay=0.01)]
    opt = optimizers.Adam([dict(params=params[:2], **kws[0]), dict(params=params[2:], **kws[1])], betas=A, eps=1e-8)
    for p, f in zip(params, fams):
        p.grad = f.g.to(device)
        _inject(opt, p, f, 5, False)
    opt.step()
    torch.cuda.synchronize()
    for i, (p, f) in enumerate(zip(params, fams)):
        ref = R.step("adam", f, D, False, 5, betas=A, eps=1e-8, grad_scale=1.0, **kws[i // 2])
        _check_step(f"group {i // 2} n={p.numel()}", _state(opt, p), ref)
        assert opt.state[p]["step"] == 5


def test_a_parameter_without_gradient_is_left_alone_and_a_late_one_is_refused(device):
    fams = [R.family(n, 1, 30 + i) for i, n in enumerate((257, 4097))]
    params = [f.p.clone().to(device).requires_grad_() for f in fams]
    opt = optimizers.Adam(params, lr=1e-3)
    params[0].grad = fams[0].g.to(device)  # params[1].grad stays None
    opt.step()
    torch.cuda.synchronize()
    assert _same_bits(params[1], fams[1].p)
    assert "step" not in opt.state.get(params[1], {})
    ref = R.step("adam", fams[0], D, False, 1, lr=1e-3, betas=A, eps=1e-8, weight_decay=0, grad_scale=1.0)
    _check_step("the parameter with a gradient", _state(opt, params[0]), ref)
    # its first gradient arrives one step later than the group's: one launch cannot serve two step counts
    before = [p.detach().cpu().clone() for p in params]
    params[1].grad = fams[1].g.to(device)
    with pytest.raises(RuntimeError, match="one common step count per parameter group"):
        opt.step()
    torch.cuda.synchronize()
    assert all(_same_bits(p, b) for p, b in zip(params, before)), "a refused step changed a parameter"


def test_flat_grads_override_the_grad_attribute(device):
    """The data-parallel reducer hands the optimizer views into its flat bucket; here they start 4 bytes past a
    16-byte boundary, and ``p.grad`` holds NaN."""
    sizes = (255, 4097, 3)
    fams = [R.family(n, 2, 50 + i) for i, n in enumerate(sizes)]
    params = [f.p.clone().to(device).requires_grad_() for f in fams]
    kw = dict(lr=1e-3, betas=A, eps=1e-8, weight_decay=0.01)
    opt = optimizers.RAdam(params, **kw)
    flat = torch.zeros(sum(sizes) + 4 * len(sizes) + 1, device=device)
    off, views = 1, {}
    for p, f in zip(params, fams):
        v = flat[off:off + p.numel()]
        assert v.data_ptr() % 16 == 4
        v.copy_(f.g.to(device))
        views[p] = v
        p.grad = torch.full_like(p, float("nan"))
        _inject(opt, p, f, 2, False)
        off += p.numel()
        off += (1 - off) % 4
    opt.flat_grads = views
    opt.step()
    torch.cuda.synchronize()
    for p, f in zip(params, fams):
        _check_step(f"flat_grads n={p.numel()}", _state(opt, p), R.step("radam", f, D, False, 2, grad_scale=1.0, **kw))
        assert _same_bits(views[p], f.g)


def test_cached_and_rebuilt_chunk_tables_with_a_scheduled_lr(device):
    """Step 2 refills the same gradient tensors (the cached device table is reused), step 3 brings freshly allocated
    ones (the table is rebuilt); a scheduler changes ``lr`` in between.  Each step is checked from the state the
    device held before it."""
    sizes = (70000, 257, 1)
    kw = dict(lr=1e-3, betas=A, eps=1e-8, weight_decay=0.01)
    opt, params, _ = _optimizer(device, "adam", sizes, 1, kw, amsgrad=True, seed=70)
    tables, keep = [], []
    for t, lr in ((1, 1e-3), (2, 5e-4), (3, 2.5e-4)):
        opt.param_groups[0]["lr"] = lr
        new = [R.family(n, 2, 70 + 10 * t + i).g.to(device) for i, n in enumerate(sizes)]
        for p, g in zip(params, new):
            if t == 2:
                p.grad.copy_(g)  # in place: same pointers
            else:
                keep.append(p.grad)  # alive, so that the fresh tensor cannot take its address
                p.grad = g
        snaps = [_snapshot(opt, p, p.grad) for p in params]
        opt.step()
        torch.cuda.synchronize()
        tables.append(opt._dev[0]["table_dev"])
        for p, s in zip(params, snaps):
            ref = R.step("adam", s, D, True, t, grad_scale=1.0, **dict(kw, lr=lr))
            _check_step(f"step {t} n={p.numel()}", _state(opt, p), ref)
            assert opt.state[p]["step"] == t
    assert tables[1] is tables[0], "the same gradient pointers did not take the cached table"
    assert tables[2] is not tables[1], "new gradient pointers did not rebuild the table"


# ------------------------------------------------------------------------------------------ captured step
@pytest.mark.parametrize("kind", ["adam", "radam"])
def test_captured_step_equals_an_eager_twin_bit_for_bit(kind, device):
    """One eager step, ``reserve_for_capture()``, ``step()`` captured; three replays, each after new gradient values
    written in place and ``prepare()`` -- against four eager steps of a twin.  The graph is one chain of nodes."""
    sizes = (70000, 257, 3)
    kw = dict(lr=1e-3, betas=A, eps=1e-8, weight_decay=0.01)
    grads = [[R.family(n, 2, 80 + 10 * k + i).g.to(device) for i, n in enumerate(sizes)] for k in range(4)]
    opts = []
    for _ in range(2):
        opt, params, _ = _optimizer(device, kind, sizes, 1, kw, amsgrad=True, grad_scale=0.5, seed=80)
        for p, g in zip(params, grads[0]):
            p.grad = g.clone()
        opt.step()
        opts.append((opt, params))
    (eager, pe), (graphed, pg) = opts
    torch.cuda.synchronize()
    graphed.reserve_for_capture()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.step()
    for k in (1, 2, 3):
        for a, b, g in zip(pe, pg, grads[k]):
            a.grad.copy_(g)
            b.grad.copy_(g)
        eager.step()
        graphed.prepare()
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(pe, pg):
        assert eager.state[a]["step"] == graphed.state[b]["step"] == 4
        for x, y in zip(_state(eager, a), _state(graphed, b)):
            assert (x is None and y is None) or _same_bits(x, y)
        assert bool(torch.isfinite(b).all())


# ------------------------------------------------------------------------------------------ the C entry points
class Band:
    """``values`` as a float32 view inside a sentinel-filled buffer, ``off`` floats past a 16-byte boundary, with
    GUARD floats of sentinel on each side."""

    def __init__(self, values, device, off=1):
        n = values.numel()
        self.buf = torch.full((GUARD + off + n + GUARD,), SENTINEL, dtype=torch.int32, device=device)
        self.lo, self.hi = GUARD + off, GUARD + off + n
        self.view = self.buf[self.lo:self.hi].view(torch.float32)
        self.view.copy_(values.to(device))
        assert self.view.data_ptr() % 16 == 4 * off and self.view.numel() == n

    def intact(self):
        return bool((self.buf[:self.lo] == SENTINEL).all()) and bool((self.buf[self.hi:] == SENTINEL).all())


class Table:
    """A hand-built device table of ``pwg_opt_chunk`` records, one chunk per ``Family``; ``with_vmax[i]`` False
    leaves the record's ``vmax`` NULL."""

    def __init__(self, fams, with_vmax, device):
        self.fams, self.with_vmax = fams, with_vmax
        self.bands = [[Band(x, device) for x in (f.p, f.g, f.m, f.v, f.vmax)] for f in fams]
        rows = []
        for f, b, x in zip(fams, self.bands, with_vmax):
            ptr = [band.view.data_ptr() for band in b]
            rows.append(ptr[:4] + [ptr[4] if x else 0, f.p.numel()])
            assert f.p.numel() == b[0].view.numel() <= R.CLIP_CHUNK
        self.dev = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(device)
        assert self.dev.shape == (len(fams), 6)

    def __len__(self):
        return len(self.fams)

    def ptr(self):
        return self.dev.data_ptr()

    def check(self, what, kind, t, entry, **kw):
        torch.cuda.synchronize()
        for f, b, x in zip(self.fams, self.bands, self.with_vmax):
            x = x and kind != "radam"
            ref = R.step(kind, f, D, x, t, entry=entry, **kw)
            p, g, m, v, vmax = (band.view for band in b)
            _check_step(f"{what} n={f.p.numel()}", (p, m, v, vmax if x else None), ref)
            assert all(band.intact() for band in b), f"{what} n={f.p.numel()}: a store outside the slice"
            assert _same_bits(g, f.g), "the gradient was written"
            if not x:
                assert _same_bits(vmax, f.vmax), "vmax was written though the record does not name it"

    def unchanged(self):
        torch.cuda.synchronize()
        return all(_same_bits(band.view, x) and band.intact()
                   for f, b in zip(self.fams, self.bands) for band, x in zip(b, (f.p, f.g, f.m, f.v, f.vmax)))


@pytest.mark.parametrize("wd", [0.01, 0.0, -0.01])
@pytest.mark.parametrize("t", [1, 5, 6, 10 ** 6])
@pytest.mark.parametrize("kind", ["adam", "radam"])
def test_host_scalar_entry_points(kind, t, wd, device):
    """``pwg_adam_step`` / ``pwg_radam_step``: bias corrections and the rectification computed in C from the float32
    arguments; Adam's kernel divides ``lr`` by ``1 - b1^t`` itself.  A negative decay is AdamW's for Adam and is
    taken as it stands by RAdam's formula."""
    betas = B if t == 1 else A
    sizes = (3, 257, 4097)
    tab = Table([R.family(n, t, 90 + i) for i, n in enumerate(sizes)], (True, False, True), device)
    fn = getattr(_lib.lib(), f"pwg_{kind}_step")
    _lib.check(fn(tab.ptr(), len(tab), 1e-3, betas[0], betas[1], 1e-8, wd, t, 0.5, _stream()), kind)
    ref_kind = "adamw" if (kind == "adam" and wd < 0) else kind
    tab.check(f"pwg_{kind}_step t={t} wd={wd}", ref_kind, t, "host", lr=1e-3, betas=betas, eps=1e-8,
              weight_decay=abs(wd) if ref_kind == "adamw" else wd, grad_scale=0.5)


@pytest.mark.parametrize("kind", ["adam", "radam"])
def test_dev_entry_points_on_a_mixed_table(kind, device):
    """``pwg_*_step_dev`` on chunks of 1 .. 65536 elements, with and without ``vmax``, every base pointer 4 bytes past
    a 16-byte boundary; the 8-float record as include/pwg_kernels.h lays it out."""
    sizes = (1, 255, 256, 257, 4096, 65536)
    t, lr, betas, eps, wd, s = 6, 1e-3, A, 1e-8, 0.01, 0.5
    tab = Table([R.family(n, t, 100 + i) for i, n in enumerate(sizes)], [i % 2 == 0 for i in range(len(sizes))], device)
    if kind == "adam":
        step_size, aux = lr / (1.0 - betas[0] ** t), math.sqrt(1.0 - betas[1] ** t)
    else:
        step_size, rect = R.radam_scalars(lr, betas, t, "exact")
        aux = 1.0 if rect else 0.0
    hyper = torch.tensor([lr, betas[0], betas[1], eps, wd, step_size, aux, s], dtype=torch.float32).to(device)
    fn = getattr(_lib.lib(), f"pwg_{kind}_step_dev")
    _lib.check(fn(tab.ptr(), len(tab), hyper.data_ptr(), _stream()), kind)
    tab.check(f"pwg_{kind}_step_dev", kind, t, "dev", lr=lr, betas=betas, eps=eps, weight_decay=wd, grad_scale=s)


def test_refusals_launch_nothing(device):
    lib = _lib.lib()
    bad_shape, null = -1, -4  # PWG_ERR_BAD_SHAPE, PWG_ERR_NULL
    tab = Table([R.family(n, 5, 110 + i) for i, n in enumerate((3, 257))], (True, False), device)
    hyper = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.0, 1e-3, 1.0, 1.0], dtype=torch.float32).to(device)
    out, ws = torch.zeros(2, device=device), torch.zeros(2, device=device)
    s = _stream()
    for name in ("pwg_adam_step", "pwg_radam_step"):
        fn = getattr(lib, name)
        assert fn(tab.ptr(), 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 5, 1.0, s) == bad_shape
        assert fn(tab.ptr(), -1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 5, 1.0, s) == bad_shape
        assert fn(tab.ptr(), len(tab), 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 1.0, s) == bad_shape
        assert fn(None, len(tab), 1e-3, 0.9, 0.999, 1e-8, 0.0, 5, 1.0, s) == null
    for name in ("pwg_adam_step_dev", "pwg_radam_step_dev"):
        fn = getattr(lib, name)
        assert fn(tab.ptr(), 0, hyper.data_ptr(), s) == bad_shape
        assert fn(None, len(tab), hyper.data_ptr(), s) == null
        assert fn(tab.ptr(), len(tab), None, s) == null
    assert lib.pwg_clip_grad_norm(tab.ptr(), 0, 1.0, out.data_ptr(), ws.data_ptr(), s) == bad_shape
    assert lib.pwg_clip_grad_norm(tab.ptr(), len(tab), 0.0, out.data_ptr(), ws.data_ptr(), s) == bad_shape
    assert lib.pwg_clip_grad_norm(None, len(tab), 1.0, out.data_ptr(), ws.data_ptr(), s) == null
    assert lib.pwg_clip_grad_norm(tab.ptr(), len(tab), 1.0, None, ws.data_ptr(), s) == null
    assert lib.pwg_clip_grad_norm(tab.ptr(), len(tab), 1.0, out.data_ptr(), None, s) == null
    assert tab.unchanged() and float(out.abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------ clipping
CLIP_SIZES = (1, 255, 65535, 65536, 65537, 140000)


def _clip(device, grads, max_norm):
    dev = [g.to(device) for g in grads]
    with poison_empty():
        out = optimizers.clip_grad_norm_([(None, g) for g in dev], max_norm)
    torch.cuda.synchronize()
    return out.cpu().numpy(), [g.cpu() for g in dev]


def _coef(norm, max_norm):
    """``min(1, max_norm / (norm + 1e-6))`` in float32 from the kernel's own norm."""
    c = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))
    return c if c < np.float32(1) else np.float32(1)


@pytest.fixture(scope="module")
def clip_grads():
    """The gradient set (its norm is about 1.2e3) and its float64 reference, computed once."""
    grads = [R.family(n, 2, 120 + i).g for i, n in enumerate(CLIP_SIZES)]
    return grads, R.clip([g.to(D) for g in grads], 10.0)


@pytest.mark.parametrize("max_norm", [10.0, 1e4], ids=["clipped", "not-clipped"])
def test_clip_grad_norm(max_norm, clip_grads, device):
    grads, ref = clip_grads
    assert (float(ref.norm) > max_norm) == (max_norm == 10.0)
    out, got = _clip(device, grads, max_norm)
    _within(f"clip max_norm={max_norm}", torch.tensor(out[0]), ref.norm, ref.bnorm, "clip norm")
    want = _coef(out[0], max_norm)
    assert out[1].tobytes() == want.tobytes(), (out[1], want)
    if max_norm == 10.0:
        assert out[1] < 1
        for g, x in zip(grads, got):
            assert np.array_equal((g.numpy() * out[1]).view(np.int32), x.numpy().view(np.int32))
    else:
        assert out[1] == 1.0
        assert all(_same_bits(g, x) for g, x in zip(grads, got))
    out2, _ = _clip(device, grads, max_norm)
    assert out.tobytes() == out2.tobytes(), "two calls on equal inputs differ"


def test_clip_grad_norm_edges(device):
    sizes = (255, 65537, 3)
    zeros = [torch.zeros(n) for n in sizes]
    out, got = _clip(device, zeros, 1.0)
    assert out[0] == 0.0 and out[1] == 1.0
    assert all(_same_bits(z, x) for z, x in zip(zeros, got))
    base = [R.family(n, 2, 130 + i).g for i, n in enumerate(sizes)]
    inf = [g.clone() for g in base]
    inf[1][65536] = float("inf")  # the one element of the tensor's second chunk
    out, _ = _clip(device, inf, 1.0)
    assert out[0] == np.inf and out[1] == 0.0  # torch.nn.utils.clip_grad_norm_: max_norm / inf
    nan = [g.clone() for g in base]
    nan[1][300] = float("nan")
    out, _ = _clip(device, nan, 1.0)
    assert np.isnan(out[0])  # the caller can see it; what happens to the gradients is not pinned


def test_worst_ratios_on_the_gpu():
    """Runs last: the largest err / bound of each kind of output over the module."""
    print("worst err / bound on the GPU: " + ", ".join(f"{k}={v:.3f}" for k, v in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values())
