"""Plain references of the optimizer and gradient-clipping operations of ``csrc/reduce_optim.hip`` (Adam / AdamW /
RAdam single steps, the clipped L2 norm), written from the formulas -- torch.optim.Adam's non-fused rule, torch.optim.
AdamW's decoupled decay, the reference project's ``optimizers/radam.py:27-99`` -- not from the kernels, and importable
without a GPU.  Dtype-generic like ``tests/elementwise_refs.py``: called with float64 tensors a function is THE
reference, called with float32 tensors it is the same formula evaluated on the CPU in float32 (every scalar operation
in float32 too).

How the scalars enter (``hyper``)
---------------------------------
``"exact"``      Python doubles throughout: torch's rule.
``"as_passed"``  the kernels' contract: ``lr, b1, b2, eps, wd, grad_scale`` are the float32 values nearest to the ones
                 given (a ``float`` kernel argument, a float32 element of the 8-float device record), ``1 - b`` is taken
                 from the ROUNDED ``b``, and the host-computed scalars are rounded to float32 exactly as they are handed
                 over (``entry``):

                 * ``entry="dev"`` (``pwg_*_step_dev`` fed by ``optimizers/fused.py``): ``step_size`` and
                   ``sqrt(1 - b2^t)`` come from the UNROUNDED doubles and are rounded once;
                 * ``entry="host"`` (``pwg_adam_step`` / ``pwg_radam_step``): the C code computes them from the float32
                   arguments widened to double; Adam's kernel gets ``float(1 - b1^t)`` and divides ``lr`` by it itself
                   (one more rounding in the kernel, counted below).

The two modes differ by more than rounding noise: ``float32(0.999) = 0.99900001287``, so ``1 - b2`` is 0.00099998713,
1.29e-5 relative below 0.001, and ``exp_avg_sq`` follows torch's rule only to that (about 200 float32 ulps; ``b1 =
0.9`` gives 2.4e-7, 0.5 gives 0).  That is harmless for training and it is not rounding error of the kernel, so the GPU
is compared with ``"as_passed"``, and the distance between the modes has a bound of its own, ``mode_distance_bound``:
``|float32(b) - b| <= U b < U`` moves the factor ``1 - b`` by at most ``U / (1 - b)`` relative (6.0e-5 for 0.999;
measured 1.29e-5).

Bounds
------
Every function returns next to each value the bound of a float32 evaluation of it (``U = 2^-24``), stated in sums of
absolute values of terms -- never relative to the result: ``m'`` and the update cancel.  The ``k`` are the number of
roundings on the longest path to the output plus one (the one absorbs the second-order terms); contraction into an FMA
only removes a rounding, ``sqrtf`` and the division are correctly rounded.

    S_g   = |s g| + |wd p|                               (RAdam: |s g|; its decay acts on p)
    S_m   = b1 |m| + (1 - b1) S_g                         bound(m') = k_m U S_m
    S_v   = b2 v + (1 - b2) S_g^2                         bound(v') = bound(vmax') = k_v U S_v   (|max(a, x) - max(a, y)| <= |x - y|)
    d     = sqrt(v^) / sqrt(1 - b2^t) + eps               (RAdam rectified: sqrt(v') + eps)
    d_lo  = (sqrt(max(v^ - bound(v'), 0)) / sqrt(1 - b2^t) + eps) (1 - 4 U)      the smallest d a float32 run can form
    |D|_S = step_size S_m / d_lo
    bound(p') = U (k_p |p| + k_d |D|_S) + step_size |m'| (1 / d_lo - 1 / d)

The last term is the denominator's share: where ``s g`` and ``wd p`` cancel, ``v'`` is small against ``S_v``, the
square root of it is not relatively accurate, and no count of roundings times ``|D|_S`` covers that; elsewhere the term
is about ``k_v / 2`` further units of ``U |D|_S``.

Counts (Adam and AdamW; the longest path runs through ``g``):
    g^  = s g + wd p                    3  (product, product, sum)
    m'  : g^ 3, 1 - b1 1, (1 - b1) g^ 1, b1 m + . 1                        6 -> k_m = 7     (the product b1 m is on the
          shorter path)
    v'  : g^ twice 6, 1 - b2 1, two products 2, + b2 v 1                   10 -> k_v = 11
    p'  : p (1 - lr wd): lr wd and 1 - . 2, the product 1; the last subtraction 1 (U |p'| <= U (|p| + |D|))
                                                                            4 -> k_p = 5
          D: m' 6, m' / d 1, step_size * . 1, the last subtraction 1       9 -> k_d = 10   (+1 with entry="host":
          lr / (1 - b1^t) is formed in the kernel)
RAdam: g^ = s g is one rounding, so k_m = 5, k_v = 7; p: wd lr 1, . p 1, the sum 1, the last sum 1 -> k_p = 5;
D: m' 4, the quotient 1 (rectified), the product 1, the last sum 1 -> k_d = 8, with d_lo = (sqrt(.) + eps)(1 - 3 U).

The clip norm: ``sqrt(sum g^2)`` summed as the kernels do -- up to 256 serial terms per lane of a 64 Ki chunk, six
shuffle levels and three sums of the block tree, then the same over the per-chunk partials.  All terms are
non-negative, so the sum of squares is relatively accurate to (its depth + 1 for the square) ``U``, the root halves
that and adds its own rounding (``clip``).
"""
import collections
import math

import torch

from tests.elementwise_refs import U, f32

D = torch.float64
CLIP_CHUNK = 65536  # elements per workgroup of the clip kernels (optimizers/fused.py: CHUNK)
CLIP_EPS = 1e-6     # torch.nn.utils.clip_grad_norm_: coef = max_norm / (norm + 1e-6), clamped at 1

Step = collections.namedtuple("Step", "p m v vmax bp bm bv bvmax")   # values, then the bound of each
Clip = collections.namedtuple("Clip", "norm coef grads bnorm bcoef bgrads")


def mode_distance_bound(b1, b2):
    """``(d1, d2)``: the largest relative change of the factor ``1 - b1`` (of ``exp_avg``) and ``1 - b2`` (of
    ``exp_avg_sq``) between ``hyper="exact"`` and ``"as_passed"``: ``U / (1 - b)``.  The factor ``b`` itself and
    every other rounded scalar move by ``U`` relative."""
    return U / (1.0 - b1), U / (1.0 - b2)


def _scalars(dtype, hyper, **kw):
    """The named scalars as 0-dim tensors of ``dtype``, rounded to float32 first with ``"as_passed"``."""
    assert hyper in ("as_passed", "exact")
    r = f32 if hyper == "as_passed" else float
    return {k: torch.tensor(r(v), dtype=dtype) for k, v in kw.items()}


def _one(dtype):
    return torch.tensor(1.0, dtype=dtype)


def adam_scalars(lr, betas, t, hyper, entry="dev"):
    """``(numerator, divisor, sqrt(1 - b2^t), extra roundings)`` with ``step_size = numerator / divisor``."""
    b1, b2 = betas
    if hyper == "exact":
        return lr, 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t), 0
    if entry == "dev":
        return f32(lr / (1.0 - b1 ** t)), 1.0, f32(math.sqrt(1.0 - b2 ** t)), 0
    assert entry == "host"
    return f32(lr), f32(1.0 - f32(b1) ** t), f32(math.sqrt(1.0 - f32(b2) ** t)), 1


def adam_step(p, g, m, v, vmax, *, lr, betas, eps, weight_decay, t, grad_scale=1.0, decoupled=False,
              hyper="as_passed", entry="dev"):
    """One step of torch.optim.Adam's non-fused rule (``decoupled``: torch.optim.AdamW's) at the 1-based step ``t``;
    ``vmax`` not None is amsgrad.  Returns ``Step``; the inputs are left alone."""
    dt = p.dtype
    wd = abs(weight_decay) if decoupled else weight_decay
    assert wd >= 0
    c = _scalars(dt, hyper, lr=lr, b1=betas[0], b2=betas[1], eps=eps, wd=wd, s=grad_scale)
    num, div, aux, extra = adam_scalars(lr, betas, t, hyper, entry)
    step = torch.tensor(num, dtype=dt) / torch.tensor(div, dtype=dt)
    aux = torch.tensor(aux, dtype=dt)
    one = _one(dt)
    gh, s_g = g * c["s"], (g * c["s"]).abs()
    if decoupled:
        p0 = p * (one - c["lr"] * c["wd"])
    else:
        p0 = p
        if wd != 0:
            gh = gh + c["wd"] * p
            s_g = s_g + (c["wd"] * p).abs()
    m1 = c["b1"] * m + (one - c["b1"]) * gh
    v1 = c["b2"] * v + (one - c["b2"]) * gh * gh
    s_m = c["b1"] * m.abs() + (one - c["b1"]) * s_g
    s_v = c["b2"] * v + (one - c["b2"]) * s_g * s_g
    k_m, k_v, k_p, k_d = 7, 11, 5, 10 + extra
    bm, bv = k_m * U * s_m, k_v * U * s_v
    vv = v1 if vmax is None else torch.maximum(vmax, v1)
    d = torch.sqrt(vv) / aux + c["eps"]
    p1 = p0 - step * (m1 / d)
    d_lo = (torch.sqrt(torch.clamp(vv - bv, min=0)) / aux + c["eps"]) * (1 - 4 * U)
    bp = U * (k_p * p.abs() + k_d * step * s_m / d_lo) + step * m1.abs() * (1 / d_lo - 1 / d)
    return Step(p1, m1, v1, None if vmax is None else vv, bp, bm, bv, None if vmax is None else bv)


def radam_scalars(lr, betas, t, hyper, entry="dev"):
    """``(step_size, rectified)`` of optimizers/radam.py:63-86 of the reference project, ``lr`` included: the length
    of the approximated simple moving average ``N_sma = N_max - 2 t b2^t / (1 - b2^t)``, ``N_max = 2 / (1 - b2) - 1``;
    from ``N_sma >= 5`` on the step is rectified."""
    b1, b2 = betas
    if hyper == "as_passed" and entry == "host":
        lr, b1, b2 = f32(lr), f32(b1), f32(b2)
    b2t = b2 ** t
    n_max = 2.0 / (1.0 - b2) - 1.0
    n_sma = n_max - 2.0 * t * b2t / (1.0 - b2t)
    rectified = n_sma >= 5
    if rectified:
        step_size = lr * math.sqrt((1 - b2t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max
                                   / (n_max - 2)) / (1 - b1 ** t)
    else:
        step_size = lr / (1 - b1 ** t)
    return (f32(step_size) if hyper == "as_passed" else step_size), rectified


def radam_step_size_distance(betas, t):
    """Bound of the relative distance of RAdam's ``step_size`` between the two ``hyper`` modes.  ``N_sma = 1 + 2 mu``
    with ``mu`` the mean of the indices 0 .. t-1 under the weights ``b2^i``, so ``d mu / d b2 = Var(i) / b2`` with
    ``Var(i) <= min((t-1)^2 / 4, b2 / (1 - b2)^2)``; ``N_max`` moves by ``2 U / (1 - b2)^2``; the logarithmic
    derivative of ``(N-4)(N-2)/N`` is below ``1/(N-4) + 1/(N-2)`` for either ``N``; ``1 - b^t`` moves by at most
    ``U / (1 - b)`` relative (``t b^t / (1 - b^t) <= b / (1 - b)``).  Doubled for the second-order terms."""
    b1, b2 = betas
    d1, d2 = mode_distance_bound(b1, b2)
    _, rectified = radam_scalars(1.0, betas, t, "exact")
    rel = d1 + 2 * U  # 1 - b1^t, lr, the rounding of step_size itself
    if rectified:
        b2t = b2 ** t
        n_max = 2.0 / (1.0 - b2) - 1.0
        n_sma = n_max - 2.0 * t * b2t / (1.0 - b2t)
        dn = 2 * U * min((t - 1) ** 2 / 4.0, b2 / (1 - b2) ** 2) / b2
        dn_max = 2 * U / (1 - b2) ** 2
        rel += 0.5 * (d2 + dn * (1 / (n_sma - 4) + 1 / (n_sma - 2)) + dn_max * (1 / (n_max - 4) + 1 / (n_max - 2)))
    return 2 * rel


def radam_step(p, g, m, v, *, lr, betas, eps, weight_decay, t, grad_scale=1.0, hyper="as_passed", entry="dev"):
    """One step of the reference project's RAdam (optimizers/radam.py:27-99): both moments from the plain gradient,
    ``p -= wd lr p``, then ``p -= step_size m / (sqrt(v) + eps)`` when rectified, else ``p -= step_size m``.
    Returns ``Step`` with ``vmax`` None."""
    dt = p.dtype
    c = _scalars(dt, hyper, lr=lr, b1=betas[0], b2=betas[1], eps=eps, wd=weight_decay, s=grad_scale)
    step_size, rectified = radam_scalars(lr, betas, t, hyper, entry)
    step = torch.tensor(step_size, dtype=dt)
    one = _one(dt)
    gh = g * c["s"]
    s_g = gh.abs()
    v1 = c["b2"] * v + (one - c["b2"]) * gh * gh
    m1 = c["b1"] * m + (one - c["b1"]) * gh
    s_m = c["b1"] * m.abs() + (one - c["b1"]) * s_g
    s_v = c["b2"] * v + (one - c["b2"]) * s_g * s_g
    k_m, k_v, k_p, k_d = 5, 7, 5, 8
    bm, bv = k_m * U * s_m, k_v * U * s_v
    p0 = p + (-c["wd"] * c["lr"]) * p if weight_decay != 0 else p
    if rectified:
        d = torch.sqrt(v1) + c["eps"]
        p1 = p0 - step * (m1 / d)
        d_lo = (torch.sqrt(torch.clamp(v1 - bv, min=0)) + c["eps"]) * (1 - 3 * U)
        bp = U * (k_p * p.abs() + k_d * step * s_m / d_lo) + step * m1.abs() * (1 / d_lo - 1 / d)
    else:
        p1 = p0 - step * m1
        bp = U * (k_p * p.abs() + k_d * step * s_m)
    return Step(p1, m1, v1, None, bp, bm, bv, None)


def clip_depth(sizes):
    """Roundings on the longest path of the kernels' sum of squares over tensors of ``sizes`` elements: the square,
    the serial sums of one lane (256 lanes walk a chunk of up to 64 Ki), 6 + 3 of the block tree, then the same over
    the per-chunk partials."""
    n_chunks = sum(-(-n // CLIP_CHUNK) for n in sizes)
    lane = -(-min(max(sizes), CLIP_CHUNK) // 256)
    return 1 + lane + 9 + -(-n_chunks // 256) + 9


def clip(grads, max_norm, hyper="as_passed"):
    """``torch.nn.utils.clip_grad_norm_`` (L2): ``(total_norm, coef, scaled_grads)`` with ``coef = min(1, max_norm /
    (norm + 1e-6))``, and their bounds.  The sum of squares is relatively accurate to ``(depth + 1) U``; the norm to
    half of that plus the root's rounding plus one; ``coef`` adds the sum and the division; a scaled gradient the
    product."""
    dt = grads[0].dtype
    c = _scalars(dt, hyper, max_norm=max_norm, e=CLIP_EPS)
    sq = torch.stack([(g * g).sum() for g in grads]).sum()
    norm = torch.sqrt(sq)
    k_n = (clip_depth([g.numel() for g in grads]) + 1) / 2 + 2
    bnorm = k_n * U * norm
    raw = c["max_norm"] / (norm + c["e"])
    coef = torch.clamp(raw, max=1.0)
    k_c = k_n + 3
    bcoef = torch.where(raw * (1 - k_c * U) >= 1, torch.zeros_like(raw), k_c * U * raw)
    scaled = [g * coef for g in grads]
    return Clip(norm, coef, scaled, bnorm, bcoef, [(k_c + 2) * U * s.abs() for s in scaled])


# ------------------------------------------------------------------------------------------------- input families
Family = collections.namedtuple("Family", "p g m v vmax")


def family(n, t, seed):
    """float32 inputs of one ``n``-element tensor at step ``t``: ``p ~ N(0,1)``; ``g ~ N(0,1) 10^U(-4,1)`` with
    about one exact zero in eight; ``m ~ 0.1 N(0,1)``, ``v ~ 0.01 U(0,1)``, ``vmax = v U(0.5,2)`` (both sides of the
    max occur); all state zero at ``t = 1``."""
    gen = torch.Generator().manual_seed(seed * 1000003 + n)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * 10.0 ** (torch.rand(n, generator=gen) * 5 - 4)
    g = torch.where(torch.rand(n, generator=gen) < 0.125, torch.zeros_like(g), g)
    m = 0.1 * torch.randn(n, generator=gen)
    v = 0.01 * torch.rand(n, generator=gen)
    vmax = v * (0.5 + 1.5 * torch.rand(n, generator=gen))
    if t == 1:
        m, v, vmax = torch.zeros_like(m), torch.zeros_like(v), torch.zeros_like(vmax)
    return Family(p, g, m, v, vmax)


def step(kind, fam, dtype, amsgrad, t, hyper="as_passed", entry="dev", **kw):
    """``adam_step`` (``kind`` "adam"), its decoupled form ("adamw") or ``radam_step`` ("radam") on a ``Family``
    converted to ``dtype``; ``kw``: lr, betas, eps, weight_decay, grad_scale."""
    p, g, m, v, vmax = (x.detach().cpu().to(dtype) for x in fam)
    if kind == "radam":
        return radam_step(p, g, m, v, t=t, hyper=hyper, entry=entry, **kw)
    assert kind in ("adam", "adamw")
    return adam_step(p, g, m, v, vmax if amsgrad else None, t=t, decoupled=kind == "adamw", hyper=hyper,
                     entry=entry, **kw)


def ratio(got, ref, bound):
    """Largest ``|got - ref| / bound`` over the elements; where the bound is 0 the values must be equal (inf if
    not).  Non-finite values give inf."""
    got, ref, bound = got.detach().cpu().to(D), ref.detach().cpu().to(D), bound.detach().cpu().to(D)
    if not (bool(torch.isfinite(got).all()) and bool(torch.isfinite(ref).all())):
        return math.inf
    err = (got - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, math.inf),
                                                                          torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0
