"""CPU: the float64 references of tests/elementwise_refs.py against torch's own float64 evaluation of the same
operations (so that the GPU matrix of tests/test_elementwise_matrix_gpu.py is compared with something that is itself
checked), and the completeness check: every ``extern "C" int pwg_*`` entry point of csrc/elementwise.hip and the
reduction entry points of csrc/reduce_optim.hip must name, in ``COVERED``, the test that drives it directly."""
import importlib
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import elementwise_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = torch.float64
TIGHT = 1e-12  # two float64 evaluations of O(1) quantities over at most a few hundred terms


def _rand(*shape, seed=0):
    return torch.randn(*shape, dtype=D, generator=torch.Generator().manual_seed(seed))


def _close(a, b, tol=TIGHT):
    assert a.shape == b.shape, (a.shape, b.shape)
    err = (a - b).abs().max().item() if a.numel() else 0.0
    assert err <= tol * max(1.0, b.abs().max().item()), err


def _grad(fn, x, dy):
    x = x.detach().clone().requires_grad_(True)
    return torch.autograd.grad(fn(x), x, dy)[0]


@pytest.mark.parametrize("cip", [True, False])
@pytest.mark.parametrize("k,s,p", [(4, 2, 2), (4, 2, 0), (3, 1, 1), (1, 1, 0), (5, 3, 2), (2, 3, 0), (7, 2, 3)])
def test_avg_pool_matches_torch(k, s, p, cip):
    for t_in in (k - 1, k, k + 1, 2 * k + s, 23, 24):
        if t_in < 1 or R.avg_pool_t_out(t_in, k, s, p) < 1:
            continue
        x = _rand(3, 2, t_in, seed=t_in)
        for ceil in (False, True):
            ref = lambda v: F.avg_pool1d(v, k, s, p, ceil_mode=ceil, count_include_pad=cip)
            y, big_s = R.avg_pool1d(x, k, s, p, cip, ceil)
            _close(y, ref(x))
            _close(big_s, ref(x.abs()))
            dy = _rand(*y.shape, seed=1)
            _close(_grad(lambda v: R.avg_pool1d(v, k, s, p, cip, ceil)[0], x, dy), _grad(ref, x, dy))


@pytest.mark.parametrize("mode", ["zero", "reflect", "replicate"])
def test_pad_matches_torch(mode):
    tmode = {"zero": "constant", "reflect": "reflect", "replicate": "replicate"}[mode]
    for t_in in (1, 2, 9, 30):
        pads = [(0, 0), (3, 0), (0, 5), (2, 7), (t_in - 1, t_in - 1), (t_in + 3, 2 * t_in)]
        for pl, pr in pads:
            if mode == "reflect" and (pl >= t_in or pr >= t_in):
                continue
            x = _rand(2, 3, t_in, seed=pl + 10 * pr)
            ref = lambda v: F.pad(v, (pl, pr), mode=tmode)
            assert torch.equal(R.pad1d(x, pl, pr, mode), ref(x))
            dy = _rand(2, 3, t_in + pl + pr, seed=2)
            _close(_grad(lambda v: R.pad1d(v, pl, pr, mode), x, dy), _grad(ref, x, dy))


def test_frame_fold_is_framing_of_the_reflect_extended_signal():
    for t, pad, hop, n_cols in [(20, 8, 4, 9), (20, 19, 3, 30), (20, -5, 4, 3), (7, 6, 5, 8), (9, 0, 2, 20)]:
        x = _rand(2, t, seed=t + pad)
        ext = F.pad(x[:, None], (t - 1, t - 1), mode="reflect")[:, 0]      # one reflection on either side
        far = hop * n_cols + 2 * t
        ext = F.pad(ext, (far, far))                                       # zero beyond
        first = far + (t - 1) - pad                                        # position of index -pad
        frames = ext[:, first:first + hop * n_cols].reshape(2, n_cols, hop).transpose(1, 2)
        assert torch.equal(R.frame_fold(x, pad, hop, n_cols), frames)


def test_clamp_gradient_at_the_floor_is_torchs():
    eps = 0.25
    x = torch.tensor([0.1, 0.25, 0.5], dtype=D)
    dy = torch.tensor([2.0, 3.0, 5.0], dtype=D)
    for fn, ref in ((lambda v: R.clamp_min(v, eps), lambda v: torch.clamp(v, min=eps)),
                    (lambda v: R.log_clamp(v, eps, 2.0), lambda v: torch.log(torch.clamp(v, min=eps)) / 2.0)):
        _close(fn(x), ref(x))
        assert torch.equal(_grad(fn, x, dy), _grad(ref, x, dy))
    assert _grad(lambda v: R.clamp_min(v, eps), x, dy).tolist() == [0.0, 3.0, 5.0]
    spec = torch.tensor([[[0.5, 0.3, 0.1], [0.0, 0.4, 0.2]]], dtype=D)  # |.|^2 = 0.25 (the floor), 0.25, 0.05
    ref = lambda v: torch.sqrt(torch.clamp(v[:, :1] ** 2 + v[:, 1:] ** 2, min=eps))
    _close(R.stft_mag(spec, eps), ref(spec))
    _close(_grad(lambda v: R.stft_mag(v, eps), spec, torch.ones(1, 1, 3, dtype=D)),
           _grad(ref, spec, torch.ones(1, 1, 3, dtype=D)))


def test_instance_norm_and_upsample_match_torch():
    x = _rand(2, 3, 1)  # (torch refuses a single time step: zero variance, y = 0 and dx = 0)
    assert not R.instance_norm(x, 1e-5).any() and not _grad(lambda v: R.instance_norm(v, 1e-5), x, x).any()
    for t in (2, 63, 257):
        x = _rand(2, 3, t, seed=t)
        ref = lambda v: F.instance_norm(v, eps=1e-5)
        _close(R.instance_norm(x, 1e-5), ref(x), 1e-10)
        dy = _rand(2, 3, t, seed=3)
        _close(_grad(lambda v: R.instance_norm(v, 1e-5), x, dy), _grad(ref, x, dy), 1e-9)
    x = _rand(2, 3, 11)
    for s in (1, 3, 8):
        assert torch.equal(R.upsample_nearest(x, s), F.interpolate(x, scale_factor=s, mode="nearest"))
        add = _rand(2, 3, 11 * s, seed=s)
        assert torch.equal(R.upsample_nearest(x, s, add), F.interpolate(x, scale_factor=s, mode="nearest") + add)


@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 63), (65, 130)])
def test_spectral_norm_matches_one_training_mode_call_of_torch(rows, cols):
    torch.manual_seed(rows)
    lin = torch.nn.utils.spectral_norm(torch.nn.Linear(cols, rows, bias=False).double(), n_power_iterations=1, eps=1e-12)
    lin.train()
    w0 = lin.weight_orig.detach().clone()
    u0, v0 = lin.weight_u.detach().clone(), lin.weight_v.detach().clone()
    x = torch.eye(cols, dtype=D)
    w_t = lin(x).t()  # = the normalised weight of this call, with the graph attached
    w_r, sigma, u, v = R.spectral_norm(w0, u0, v0, True, 1e-12)
    _close(w_r, w_t.detach(), 1e-10)
    _close(u, lin.weight_u.detach(), 1e-10)
    _close(v, lin.weight_v.detach(), 1e-10)
    dy = _rand(rows, cols, seed=5)
    g_t = torch.autograd.grad(w_t, lin.weight_orig, dy)[0]
    _close(_grad(lambda w: R.spectral_norm(w, u0, v0, True, 1e-12)[0], w0, dy), g_t, 1e-9)
    # without the iteration: sigma of the given u, v
    _close(R.spectral_norm(w0, u, v, False, 1e-12)[1], torch.dot(u, w0 @ v), 1e-12)


def test_weight_norm_matches_torch():
    for shape in ((1, 1, 1), (5, 3, 21), (4, 63)):
        v, g = _rand(*shape, seed=1), _rand(shape[0], *([1] * (len(shape) - 1)), seed=2)
        _close(R.weight_norm(v, g), torch._weight_norm(v, g, 0))
        dy = _rand(*shape, seed=3)
        for i, x in enumerate((v, g)):
            ours = _grad(lambda t: R.weight_norm(*((t, g) if i == 0 else (v, t))), x, dy)
            theirs = _grad(lambda t: torch._weight_norm(*((t, g) if i == 0 else (v, t)), 0), x, dy)
            _close(ours, theirs, 1e-11)


def _tie_data(n, seed=0):
    a, b = _rand(n, seed=seed), _rand(n, seed=seed + 1)
    ties = [(1, 1), (-1, -1), (0, 0), (0, 0.5), (0.5, 0), (-0.0, 0.3), (1, -1), (-1, 1)]
    for i, (x, y) in enumerate(ties[:n]):
        a[i], b[i] = x, y
    return a, b


def test_reductions_match_torch_values_and_tie_gradients():
    a, b = _tie_data(40)
    c, scale, gout = 0.25, 1.0 / 40, torch.tensor(0.75, dtype=D)
    zeros = torch.zeros_like(a)
    torch_forms = {
        "abs_diff": lambda x, y: F.l1_loss(x, y),
        "sq_diff": lambda x, y: F.mse_loss(x, y),
        "sq": lambda x, y: (x * x).mean(),
        "sq_diff_const": lambda x, y: F.mse_loss(x, torch.full_like(x, c)),
        "sum": lambda x, y: x.mean(),
        "hinge_real": lambda x, y: -torch.mean(torch.min(x - 1, zeros)),
        "hinge_fake": lambda x, y: -torch.mean(torch.min(-x - 1, zeros)),
        "abs_diff_lrelu": lambda x, y: F.l1_loss(F.leaky_relu(x, c), F.leaky_relu(y, c)),
    }
    assert set(torch_forms) == set(R.RED_MODES)
    for mode, form in torch_forms.items():
        x, y = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        val = form(x, y)
        ours, big_s = R.reduce_value(mode, a, b, c, scale)
        _close(ours, val.detach())
        assert big_s >= ours.abs()
        gx, gy = torch.autograd.grad(val, (x, y), gout, allow_unused=True)
        da, db = R.reduce_grads(mode, a, b, c, scale, gout)
        _close(da, gx)
        if mode in R.RED_BINARY:
            _close(db, gy)
        else:
            assert db is None
    # the tie values themselves
    da, db = R.reduce_grads("abs_diff", a, b, c, 1.0, 1.0)
    assert da[:3].tolist() == [0.0, 0.0, 0.0] and db[:3].tolist() == [0.0, 0.0, 0.0]
    assert R.reduce_grads("hinge_real", a, b, c, 1.0, 1.0)[0][0].item() == -0.5
    assert R.reduce_grads("hinge_fake", a, b, c, 1.0, 1.0)[0][1].item() == 0.5
    da, db = R.reduce_grads("abs_diff_lrelu", a, b, c, 1.0, 1.0)
    assert da[3].item() == -c and db[4].item() == -c and da[5].item() == -c


def test_stretch_conv_matches_a_direct_triple_loop():
    rng = np.random.default_rng(0)
    for s, fk, pad_left in ((1, 1, 1), (2, 3, 2), (3, 5, 6), (4, 1, 8)):
        k = 2 * s + 1
        x, w = rng.standard_normal((2, 4, 5)), rng.standard_normal((fk, k))
        xs = np.repeat(x, s, axis=-1)
        y = np.zeros_like(xs)
        for c in range(4):
            for t in range(5 * s):
                for f in range(fk):
                    for j in range(k):
                        cc, u = c + f - (fk - 1) // 2, t + j - pad_left
                        if 0 <= cc < 4 and 0 <= u < 5 * s:
                            y[:, c, t] += w[f, j] * xs[:, cc, u]
        ours, big_s = R.stretch_conv(torch.from_numpy(x), torch.from_numpy(w), s, pad_left)
        _close(ours, torch.from_numpy(y))
        assert (big_s + 1e-300 >= ours.abs()).all()
        _close(R.stretch_conv(torch.from_numpy(x), torch.from_numpy(w), s, pad_left, "leaky_relu", 0.2)[0],
               F.leaky_relu(torch.from_numpy(y), 0.2))


def test_small_formulas():
    z = _rand(2, 6, 5)
    _close(R.gate(z), torch.tanh(z[:, :3]) / (1 + torch.exp(-z[:, 3:])))
    e = torch.exp(z[:, :3])
    _close(R.tade_gate(z, True), e / e.sum(1, keepdim=True) * torch.tanh(z[:, 3:]))
    _close(R.tade_gate(z, False), torch.tanh(z[:, 3:]) / (1 + torch.exp(-z[:, :3])))
    big = 90 * torch.sign(z)
    assert torch.isfinite(R.gate(big)).all() and torch.isfinite(R.tade_gate(big, True)).all()
    xn, cg = _rand(2, 3, 4), _rand(2, 6, 8, seed=1)
    y, big_s = R.tade_modulate(xn, cg, 2)
    _close(y, cg[:, :3] * F.interpolate(xn, scale_factor=2, mode="nearest") + cg[:, 3:])
    assert (big_s >= y.abs() - 1e-15).all()
    pcm = R.wave_to_pcm16(torch.tensor([0.5 / 32767, 1.5 / 32767, 2.5 / 32767, -0.5 / 32767, 1.0, -1.0, 1.5, -1.5, 0.0]))
    assert pcm.tolist() == [0, 2, 2, 0, 32767, -32767, 32767, -32767, 0]
    x = _rand(2, 5, 3)
    mean, scale = _rand(3, seed=1), _rand(3, seed=2).abs() + 0.5
    assert torch.equal(R.normalize_transpose(x), x.transpose(1, 2))
    _close(R.normalize_transpose(x, mean, scale)[1, 2, 4], (x[1, 4, 2] - mean[2]) / scale[2])
    y = _rand(7)
    for act in (None, "leaky_relu", "relu", "tanh"):
        pre = _rand(7, seed=4).requires_grad_(True)
        out = R.activation(pre, act, 0.2)
        g = torch.autograd.grad(out, pre, y)[0]
        _close(R.act_backward(y, out.detach(), act, 0.2, 0.5), 0.5 * g)


# ------------------------------------------------------------------------------------------------ completeness
def _entry_points():
    csrc = os.path.join(ROOT, "parallelwavegan_amd", "csrc")
    pat = re.compile(r'^extern "C" int (pwg_\w+)\(', re.M)
    names = pat.findall(open(os.path.join(csrc, "elementwise.hip")).read())
    names += [n for n in pat.findall(open(os.path.join(csrc, "reduce_optim.hip")).read())
              if n.startswith(("pwg_reduce_", "pwg_multi_reduce_"))]
    return names


def test_every_entry_point_names_the_test_that_drives_it():
    names = _entry_points()
    assert len(names) > 40 and "pwg_reduce_forward" in names and "pwg_pad1d_backward" in names, names
    gpu = importlib.import_module("tests.test_elementwise_matrix_gpu")
    missing = [n for n in names if n not in gpu.COVERED]
    assert not missing, f"entry points with no direct test: {missing}"
    stale = [n for n in gpu.COVERED if n not in names]
    assert not stale, f"COVERED names entry points that no longer exist: {stale}"
    for name, where in gpu.COVERED.items():
        if where.endswith(".py"):
            assert os.path.exists(os.path.join(ROOT, where)), f"{name}: {where} does not exist"
        else:
            fn = getattr(gpu, where, None)
            assert callable(fn) and where.startswith("test_"), f"{name}: no test function {where}"
            assert any(m.name == "gpu" for m in getattr(fn, "pytestmark", [])), f"{where} is not marked gpu"
