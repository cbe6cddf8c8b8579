"""Plain torch / numpy references of the element-wise, norm and reduction operations of ``csrc/elementwise.hip`` and
``csrc/reduce_optim.hip``, written from the formulas (not from the kernels) and importable without a GPU.

Every function is dtype-generic: called with float64 tensors it is THE reference, called with float32 tensors it is the
"float32 CPU evaluation of the same formula" whose own distance from float64 sizes the tolerance of the operations that
pass through ``tanh``, ``exp``, ``log``, ``sqrt``, ``rsqrt`` or a division.  Backward passes come from autograd on these
functions; where the gradient at a tie is a choice, it is written explicitly (``clamp_min``, ``reduce_grads``) next to
the line of the reference project whose torch expression fixes it.

Operations that are sums return ``(y, S)``: ``S`` is the sum of the absolute values of the terms of each output
element, the quantity the forward-error bound ``(n_terms + 4) * 2^-24 * S`` is stated in.
"""
import numpy as np
import torch
import torch.nn.functional as F

D = torch.float64
U = 2.0 ** -24  # unit roundoff of float32

RED_MODES = ("abs_diff", "sq_diff", "sq", "sq_diff_const", "sum", "hinge_real", "hinge_fake", "abs_diff_lrelu")
RED_BINARY = ("abs_diff", "sq_diff", "abs_diff_lrelu")


def f32(v):
    """The float32 value nearest to ``v`` as a Python float (what a ``float`` kernel argument receives)."""
    return float(np.float32(v))


def ulp32(ref):
    """Spacing of float32 at ``|ref|`` (2^-149 below the smallest normal number)."""
    return torch.clamp(ref.abs().double(), min=2.0 ** -126) * 2.0 ** -23


# ---------------------------------------------------------------------------------------------- autograd helpers
def run(fn, ins, req, dy=None, dtype=D):
    """``fn(*ins)`` in ``dtype`` on the CPU and, with ``dy``, its gradients for the inputs flagged in ``req``.
    Returns ``[y, grads...]`` (``y`` may be a tuple ``(y, S)``: the gradient is taken of its first element)."""
    xs = [None if t is None else t.detach().cpu().to(dtype).requires_grad_(bool(r)) for t, r in zip(ins, req)]
    out = fn(*xs)
    y = out[0] if isinstance(out, tuple) else out
    res = [tuple(o.detach() for o in out) if isinstance(out, tuple) else y.detach()]
    if dy is not None and any(req):
        gs = torch.autograd.grad(y, [x for x, r in zip(xs, req) if r], dy.detach().cpu().to(dtype))
        res += [g.detach() for g in gs]
    return res


def run_abs(fn, ins, req, dy=None):
    """``run`` at the absolute values of the inputs and of ``dy``: for an operation whose outputs and gradients are
    sums of products of its inputs with non-negative structure coefficients (gathers, windows, correlations) this is
    ``S`` of every output and gradient element."""
    return run(fn, [None if t is None else t.abs() for t in ins], req, None if dy is None else dy.abs())


class _ClampMin(torch.autograd.Function):
    """``torch.clamp(x, min=eps)``; the gradient passes where ``x >= eps`` -- AT the floor too: torch's rule for the
    ``torch.clamp(..., min=...)`` of losses/stft_loss.py:40 and losses/mel_loss.py:105,108 of the reference project."""

    @staticmethod
    def forward(ctx, x, eps):
        ctx.save_for_backward(x)
        ctx.eps = eps
        return torch.where(x > eps, x, torch.full_like(x, eps))

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return torch.where(x >= ctx.eps, g, torch.zeros_like(g)), None


def clamp_min(x, eps):
    return _ClampMin.apply(x, eps)


# ---------------------------------------------------------------------------------------------- pooling / padding
def avg_pool_t_out(t_in, k, s, p, ceil_mode=False):
    """Number of windows; ``ceil_mode`` is torch's: one more window when the stride leaves a remainder, provided it
    starts inside the signal or its left padding."""
    n = t_in + 2 * p - k
    t_out = (-(-n // s) if ceil_mode else n // s) + 1
    if ceil_mode and (t_out - 1) * s >= t_in + p:
        t_out -= 1
    return t_out


def avg_pool1d(x, k, s, p, count_include_pad, ceil_mode=False):
    """Windows of ``k`` with stride ``s`` over ``x`` zero-padded by ``p`` on both sides.  torch's divisor: with
    ``count_include_pad`` the window's length clipped at ``t_in + p`` (the padding counts, positions past it -- which
    only a ``ceil_mode`` window reaches -- do not), without it the number of window positions inside the signal.
    Returns ``(y, S)``."""
    t_in = x.shape[-1]
    t_out = avg_pool_t_out(t_in, k, s, p, ceil_mode)
    start = torch.arange(t_out) * s - p
    if count_include_pad:
        div = torch.clamp(start + k, max=t_in + p) - start
    else:
        div = torch.clamp(start + k, max=t_in) - torch.clamp(start, min=0)
    div = div.to(x.dtype)

    def pool(v):
        vp = torch.cat([v.new_zeros(v.shape[:-1] + (p,)), v, v.new_zeros(v.shape[:-1] + (p + k,))], dim=-1)
        return vp.unfold(-1, k, s)[..., :t_out, :].sum(-1) / div

    return pool(x), pool(x.detach().abs())


def pad_index(t_in, pl, pr, mode):
    """Source index in the signal of every position of the padded frame, and whether it reads the signal at all."""
    j = torch.arange(-pl, t_in + pr)
    inside = (j >= 0) & (j < t_in)
    if mode == "zero":
        return torch.clamp(j, 0, t_in - 1), inside
    if mode == "reflect":
        assert pl < t_in and pr < t_in
        return torch.where(j < 0, -j, torch.where(j >= t_in, 2 * (t_in - 1) - j, j)), torch.ones_like(inside)
    assert mode == "replicate"
    return torch.clamp(j, 0, t_in - 1), torch.ones_like(inside)


def pad1d(x, pl, pr, mode):
    src, reads = pad_index(x.shape[-1], pl, pr, mode)
    y = x.index_select(-1, src)
    return torch.where(reads, y, torch.zeros_like(y))


def frame_fold(x, pad, hop, n_cols):
    """(B, T) -> (B, hop, n_cols): ``y[b][c][n] = xe[n * hop + c - pad]`` where ``xe`` is ``x`` extended by ONE
    reflection on either side (``xe[-j] = x[j]``, ``xe[T-1+j] = x[T-1-j]``, ``1 <= j <= T-1``) and zero beyond."""
    t = x.shape[-1]
    j = (torch.arange(n_cols)[None, :] * hop + torch.arange(hop)[:, None] - pad).reshape(-1)
    valid = (j > -t) & (j < 2 * t - 1)
    src = torch.where(j < 0, -j, torch.where(j >= t, 2 * (t - 1) - j, j))
    src = torch.where(valid, src, torch.zeros_like(src))
    y = x.index_select(-1, src)
    y = torch.where(valid, y, torch.zeros_like(y))
    return y.reshape(x.shape[0], hop, n_cols)


# ---------------------------------------------------------------------------------------------- spectral-loss pieces
def stft_mag(spec, eps):
    """(B, 2 bins, frames), rows [real | imaginary] -> sqrt(clamp(re^2 + im^2, min=eps))."""
    bins = spec.shape[1] // 2
    re, im = spec[:, :bins], spec[:, bins:]
    return torch.sqrt(clamp_min(re * re + im * im, eps))


def log_clamp(x, eps, log_div):
    return torch.log(clamp_min(x, eps)) / log_div


# ---------------------------------------------------------------------------------------------- gates
def gate(z):
    c = z.shape[1] // 2
    return torch.tanh(z[:, :c]) * torch.sigmoid(z[:, c:])


def tade_gate(z, use_softmax):
    c = z.shape[1] // 2
    a = torch.softmax(z[:, :c], dim=1) if use_softmax else torch.sigmoid(z[:, :c])
    return a * torch.tanh(z[:, c:])


def upsample_nearest(x, s, add=None):
    y = torch.repeat_interleave(x, s, dim=-1)
    return y if add is None else y + add


def tade_modulate(xn, cg, s):
    """``cg[:, :C] * up(xn) + cg[:, C:]``.  Returns ``(y, S)``."""
    c = xn.shape[1]
    up = torch.repeat_interleave(xn, s, dim=-1)
    y = cg[:, :c] * up + cg[:, c:]
    return y, (cg[:, :c] * up).detach().abs() + cg[:, c:].detach().abs()


def activation(v, act, slope):
    if act is None or act == "none":
        return v
    if act == "leaky_relu":
        return torch.where(v > 0, v, v * slope)
    if act == "relu":
        return torch.where(v > 0, v, torch.zeros_like(v))
    assert act == "tanh"
    return torch.tanh(v)


def act_backward(dy, y, act, slope, scale):
    """``dy * scale * act'``, the derivative expressed through the activation's OUTPUT ``y``."""
    if act is None or act == "none":
        d = torch.ones_like(dy)
    elif act == "leaky_relu":
        d = torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope))
    elif act == "relu":
        d = (y > 0).to(dy.dtype)
    else:
        d = 1 - y * y
    return dy * scale * d


def stretch_conv(x, w, s, pad_left, act=None, slope=0.0):
    """x (B, C, T), w (F, k): nearest stretch by ``s`` along time, then the correlation
    ``y[b][c][t] = sum_f sum_j w[f][j] xs[b][c + f - (F-1)/2][t + j - pad_left]`` with zeros outside ``xs`` on both
    axes, then the activation.  Returns ``(y, S)``, ``S`` of the sum before the activation."""
    fk, k = w.shape
    pf = (fk - 1) // 2

    def corr(xv, wv):
        xs = torch.repeat_interleave(xv, s, dim=-1)
        xs = F.pad(xs[:, None], (pad_left, k - 1 - pad_left, pf, pf))
        return F.conv2d(xs, wv[None, None])[:, 0]

    return activation(corr(x, w), act, slope), corr(x.detach().abs(), w.detach().abs())


def add3_div(a, b, c, div):
    v = a + b
    if c is not None:
        v = v + c
    return v / div


# ---------------------------------------------------------------------------------------------- norms
def instance_norm(x, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps)


def weight_norm(v, g):
    """Old-style weight norm over dim 0: ``w[i] = g[i] * v[i] / |v[i]|``."""
    n0 = v.shape[0]
    norm = torch.sqrt((v.reshape(n0, -1) ** 2).sum(1)).reshape((n0,) + (1,) * (v.dim() - 1))
    return g.reshape(norm.shape) * v / norm


def _normalize(x, eps):
    return x / torch.clamp(torch.sqrt((x * x).sum()), min=eps)


def spectral_norm(w, u, v, do_iter, eps):
    """One power iteration (``v = n(W^T u)``, ``u = n(W v)``, ``n(x) = x / max(|x|, eps)``) when ``do_iter``, then
    ``sigma = u^T W v`` with ``u``, ``v`` detached and ``w / sigma``.  Returns ``(w_sn, sigma, u, v)``."""
    wm = w.reshape(w.shape[0], -1)
    with torch.no_grad():
        u, v = u.detach().to(w.dtype), v.detach().to(w.dtype)
        if do_iter:
            v = _normalize(wm.t() @ u, eps)
            u = _normalize(wm @ v, eps)
    sigma = torch.dot(u, wm @ v)
    return w / sigma, sigma, u, v


# ---------------------------------------------------------------------------------------------- reductions
def _lrelu(v, c):
    return torch.where(v > 0, v, v * c)


def reduce_terms(mode, a, b, c):
    """The summand of each of the eight reductions and the sum of absolute values of ITS terms (the two
    activations of ``abs_diff_lrelu`` are rounded before they are subtracted, so they are its terms)."""
    if mode == "abs_diff":
        t = (a - b).abs()
    elif mode == "sq_diff":
        t = (a - b) ** 2
    elif mode == "sq":
        t = a * a
    elif mode == "sq_diff_const":
        t = (a - c) ** 2
    elif mode == "sum":
        t = a
    elif mode == "hinge_real":  # -min(x - 1, 0)   losses/adversarial_loss.py:120
        t = -torch.clamp(a - 1, max=0)
    elif mode == "hinge_fake":  # -min(-x - 1, 0)  losses/adversarial_loss.py:123
        t = -torch.clamp(-a - 1, max=0)
    else:
        assert mode == "abs_diff_lrelu"
        la, lb = _lrelu(a, c), _lrelu(b, c)
        return (la - lb).abs(), la.abs() + lb.abs()
    return t, t.abs()


def reduce_value(mode, a, b, c, scale):
    """``scale * sum term`` and its ``S`` (0-dim tensors)."""
    t, s = reduce_terms(mode, a, b, c)
    return scale * t.sum(), abs(scale) * s.sum()


def reduce_grads(mode, a, b, c, scale, gout):
    """``(da, db)`` of ``scale * sum term`` for the upstream gradient ``gout``, the subgradients at ties explicit:

    * ``|a - b|`` at ``a == b``: 0 (``F.l1_loss``: losses/feat_match_loss.py:47, losses/stft_loss.py:82; torch
      differentiates ``abs`` with ``sign``, and ``sign(0) = 0``);
    * the hinge ``-min(x - 1, 0)`` at ``x == 1`` (``-min(-x - 1, 0)`` at ``x == -1``): -1/2 (+1/2) --
      losses/adversarial_loss.py:120,123 take ``torch.min`` of two TENSORS, whose gradient is shared equally at a tie;
    * ``leaky_relu`` at 0: the slope (torch: ``x > 0 ? 1 : slope``), so ``|lrelu(a) - lrelu(b)|`` at ``a == 0`` has
      ``d/da = sign(lrelu(a) - lrelu(b)) * slope``."""
    one, zero = torch.ones_like(a), torch.zeros_like(a)
    db = None
    if mode == "abs_diff":
        da = torch.sign(a - b)
        db = -da
    elif mode == "sq_diff":
        da = 2 * (a - b)
        db = -da
    elif mode == "sq":
        da = 2 * a
    elif mode == "sq_diff_const":
        da = 2 * (a - c)
    elif mode == "sum":
        da = one
    elif mode == "hinge_real":
        da = torch.where(a < 1, -one, torch.where(a == 1, -0.5 * one, zero))
    elif mode == "hinge_fake":
        da = torch.where(a > -1, one, torch.where(a == -1, 0.5 * one, zero))
    else:
        sg = torch.sign(_lrelu(a, c) - _lrelu(b, c))
        da = sg * torch.where(a > 0, one, c * one)
        db = -sg * torch.where(b > 0, one, c * one)
    k = gout * scale
    return k * da, (None if db is None else k * db)


# ---------------------------------------------------------------------------------------------- inference helpers
def wave_to_pcm16(x):
    """``rint(clip(x, -1, 1) * 32767)`` evaluated in float32 (round half to even), as int16."""
    v = np.clip(np.asarray(x, dtype=np.float32), np.float32(-1), np.float32(1)) * np.float32(32767)
    return torch.from_numpy(np.rint(v).astype(np.int16))


def normalize_transpose(x, mean=None, scale=None):
    """(B, T, C) -> (B, C, T), ``(x - mean[c]) / scale[c]`` when statistics are given."""
    if mean is not None:
        x = (x - mean) / scale
    return x.transpose(1, 2)


def concat_channels(a, b):
    return torch.cat((a, b), dim=1)
