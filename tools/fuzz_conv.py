"""Randomised parity sweep of the conv1d family (forward, data gradient, weight/bias gradient) against
torch CPU fp32, with PWG_POISON_LDS=1 recommended (stale-LDS hazards).  GPU box only.
usage: fuzz_conv.py [n_cases] [seed] [epilogue]      (epilogue: the second sweep, run_epilogue)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from parallelwavegan_amd import ops

RTOL = 5e-5


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().double()
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-12)


def run(n_cases, seed):
    """Returns the list of failing cases (description, errors)."""
    rng = np.random.RandomState(seed)
    dev = torch.device("cuda:0")
    bad = []
    for case in range(n_cases):
        transposed = rng.rand() < 0.25
        groups = int(rng.choice([1, 1, 1, 2, 4, 16]))
        cin = groups * int(rng.choice([1, 2, 3, 8, 16, 20, 32, 64, 96]))
        cout = groups * int(rng.choice([1, 2, 4, 8, 16, 24, 32, 64, 128]))
        if cin > 1024 or cout > 1024:
            continue
        b = int(rng.choice([1, 2, 3, 5]))
        slope = [None, 0.1, 0.2, 0.0][rng.randint(4)]
        g = torch.Generator().manual_seed(case)
        if transposed:
            stride = int(rng.choice([1, 2, 3, 4, 5, 8]))
            k = int(rng.choice([stride, 2 * stride, 2 * stride + 1, stride + 3]))
            pad = int(rng.randint(0, max(1, k // 2)))
            out_pad = int(rng.randint(0, stride)) if stride > 1 else 0
            t = int(rng.choice([1, 5, 17, 33, 64, 100, 257]))
            t_out = (t - 1) * stride - 2 * pad + k + out_pad
            if t_out <= 0 or groups > 4:
                continue
            x = torch.randn(b, cin, t, generator=g, requires_grad=True)
            w = (torch.randn(cin, cout // groups, k, generator=g) / (cin // groups * k) ** 0.5).requires_grad_()
            bias = torch.randn(cout, generator=g, requires_grad=True)
            xa = F.leaky_relu(x, slope) if slope is not None else x
            y_ref = F.conv_transpose1d(xa, w, bias, stride=stride, padding=pad, output_padding=out_pad, groups=groups)
            desc = ops.make_conv_desc(b, cin, cout, t, t_out, k, stride, 1, pad, groups, transposed=True,
                                      pre_act="leaky_relu" if slope is not None else None, pre_slope=slope or 0.0)
        elif rng.rand() < 0.3:
            # (k, 1) Conv2d over (rows, width): the period-discriminator pattern, incl. long reductions over
            # few columns (split-K candidates)
            width = int(rng.choice([2, 3, 5, 7, 11]))
            cin = int(rng.choice([1, 32, 128, 512, 1024]))
            cout = int(rng.choice([1, 32, 128, 1024]))
            groups = 1
            k = int(rng.choice([3, 5]))
            stride = int(rng.choice([1, 3]))
            pad = (k - 1) // 2
            h = int(rng.choice([4, 10, 21, 51, 90]))
            h_out = (h + 2 * pad - k) // stride + 1
            if h_out <= 0:
                continue
            b = int(rng.choice([1, 2, 4]))
            x = torch.randn(b, cin, h, width, generator=g, requires_grad=True)
            w = (torch.randn(cout, cin, k, 1, generator=g) / (cin * k) ** 0.5).requires_grad_()
            bias = torch.randn(cout, generator=g, requires_grad=True)
            xa = F.leaky_relu(x, slope) if slope is not None else x
            y_ref = F.conv2d(xa, w, bias, stride=(stride, 1), padding=(pad, 0))
            desc = ops.make_conv_desc(b, cin, cout, h, h_out, k, stride, 1, pad, 1, width=width,
                                      pre_act="leaky_relu" if slope is not None else None, pre_slope=slope or 0.0)
            t = h
        else:
            k = int(rng.choice([1, 2, 3, 5, 7, 9, 11, 15, 41]))
            stride = int(rng.choice([1, 1, 1, 2, 3, 4]))
            dil = int(rng.choice([1, 1, 2, 3, 5, 9, 27])) if stride == 1 else 1
            pad = int(rng.choice([0, (k - 1) // 2 * dil, (k - 1) * dil]))
            t = int(rng.choice([(k - 1) * dil + 1, 31, 64, 97, 128, 200, 400, 777, 1500]))
            t_out = (t + 2 * pad - dil * (k - 1) - 1) // stride + 1
            if t_out <= 0 or t < (k - 1) * dil + 1 - 2 * pad:
                continue
            x = torch.randn(b, cin, t, generator=g, requires_grad=True)
            w = (torch.randn(cout, cin // groups, k, generator=g) / (cin // groups * k) ** 0.5).requires_grad_()
            bias = torch.randn(cout, generator=g, requires_grad=True)
            xa = F.leaky_relu(x, slope) if slope is not None else x
            y_ref = F.conv1d(xa, w, bias, stride=stride, padding=pad, dilation=dil, groups=groups)
            desc = ops.make_conv_desc(b, cin, cout, t, t_out, k, stride, dil, pad, groups,
                                      pre_act="leaky_relu" if slope is not None else None, pre_slope=slope or 0.0)
        dy = torch.randn(y_ref.shape, generator=g)
        y_ref.backward(dy)
        xd, wd, bd, dyd = (v.detach().to(dev).contiguous() for v in (x, w, bias, dy))
        if x.dim() == 4:  # device side works on (B, C, rows * width)
            xd, dyd = xd.reshape(b, cin, -1), dyd.reshape(b, cout, -1)
        tag = (f"case {case}: tr={int(transposed)} B={b} Cin={cin} Cout={cout} T={t}->{y_ref.shape[-1]} k={k} "
               f"s={stride} g={groups} slope={slope}")
        try:
            y = ops.conv1d_forward(desc, xd, ops.pack_weight(desc, wd), bd)
            dx = ops.conv1d_backward_data(desc, dyd, ops.pack_weight_bwd(desc, wd), xd)
            dw, db = ops.conv1d_backward_weight(desc, xd, dyd, tuple(w.shape))
            if x.dim() == 4:
                y, dx = y.reshape(y_ref.shape), dx.reshape(x.shape)
        except RuntimeError as e:
            if "unsupported" in str(e).lower() or "dilation with stride" in str(e):
                continue
            bad.append((tag, "exception " + str(e)[:120]))
            continue
        errs = dict(y=rel(y, y_ref), dx=rel(dx, x.grad), dw=rel(dw, w.grad), db=rel(db, bias.grad))
        worst = max(errs.values())
        if not (worst <= RTOL):
            bad.append((tag, {k2: f"{v:.2e}" for k2, v in errs.items()}))
    return bad


def _act64(t, act, slope):
    if act == "leaky_relu":
        return F.leaky_relu(t, slope)
    if act == "relu":
        return F.relu(t)
    return torch.tanh(t) if act == "tanh" else t


def _view_at(t, dev, off):
    """``t`` on the device as a contiguous view that starts ``off`` floats past a 16-byte boundary."""
    buf = torch.empty(t.numel() + off, device=dev, dtype=torch.float32)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    return v


def epilogue_cases(n_cases, seed):
    """The cases of ``run_epilogue`` (host only): the geometry of ``run`` with every fused epilogue term drawn at random,
    pad modes and causal padding on plain width-1 cases, and a coin flip for the 4-byte misalignment.  Yields dicts;
    a case that the geometry filters of ``run`` drop is not yielded."""
    rng = np.random.RandomState(seed)
    for case in range(n_cases):
        transposed = rng.rand() < 0.25
        groups = int(rng.choice([1, 1, 1, 2, 4, 16]))
        cin = groups * int(rng.choice([1, 2, 3, 8, 16, 20, 32, 64, 96]))
        cout = groups * int(rng.choice([1, 2, 4, 8, 16, 24, 32, 64, 128]))
        b = int(rng.choice([1, 2, 3, 5]))
        # epilogue terms (drawn before any geometry filter: a dropped case does not shift the terms of the others)
        c = dict(case=case, transposed=transposed, has_bias=rng.rand() < 0.7, has_add1=rng.rand() < 0.5,
                 has_add2=rng.rand() < 0.4, out_mul=float(np.float32([1.0, 0.5 ** 0.5, 1.7][rng.randint(3)])),
                 out_div=[1.0, 2.0, 3.0][rng.randint(3)])
        c["post_act"], c["post_slope"] = [(None, 0.0), ("leaky_relu", 0.2), ("tanh", 0.0)][rng.randint(3)]
        c["pre_act"], c["pre_slope"] = [(None, 0.0), ("leaky_relu", 0.1), ("leaky_relu", 0.0), ("relu", 0.0)][rng.randint(4)]
        pad_mode = ["zero", "zero", "zero", "zero", "reflect", "replicate"][rng.randint(6)]
        causal = rng.rand() < 0.3
        c["off"] = int(rng.rand() < 0.5)
        c["weight_grads"] = rng.rand() < 0.4
        if cin > 1024 or cout > 1024:
            continue
        width, dil, pad_right, out_pad = 1, 1, None, 0
        if transposed:
            stride = int(rng.choice([1, 2, 3, 4, 5, 8]))
            k = int(rng.choice([stride, 2 * stride, 2 * stride + 1, stride + 3]))
            pad = int(rng.randint(0, max(1, k // 2)))
            out_pad = int(rng.randint(0, stride)) if stride > 1 else 0
            t = int(rng.choice([1, 5, 17, 33, 64, 100, 257]))
            t_out = (t - 1) * stride - 2 * pad + k + out_pad
            if t_out <= 0 or groups > 4:
                continue
            pad_mode = "zero"
        elif rng.rand() < 0.3:
            # (k, 1) Conv2d over (rows, width), as in ``run``
            width = int(rng.choice([2, 3, 5, 7, 11]))
            cin = int(rng.choice([1, 32, 128, 512, 1024]))
            cout = int(rng.choice([1, 32, 128, 1024]))
            groups = 1
            k = int(rng.choice([3, 5]))
            stride = int(rng.choice([1, 3]))
            pad = (k - 1) // 2
            t = int(rng.choice([4, 10, 21, 51, 90]))
            t_out = (t + 2 * pad - k) // stride + 1
            if t_out <= 0:
                continue
            b = int(rng.choice([1, 2, 4]))
            pad_mode = "zero"
        else:
            k = int(rng.choice([1, 2, 3, 5, 7, 9, 11, 15, 41]))
            stride = int(rng.choice([1, 1, 1, 2, 3, 4]))
            dil = int(rng.choice([1, 1, 2, 3, 5, 9, 27])) if stride == 1 else 1
            pad = int(rng.choice([0, (k - 1) // 2 * dil, (k - 1) * dil]))
            t = int(rng.choice([(k - 1) * dil + 1, 31, 64, 97, 128, 200, 400, 777, 1500]))
            t_out = (t + 2 * pad - dil * (k - 1) - 1) // stride + 1
            if t_out <= 0 or t < (k - 1) * dil + 1 - 2 * pad:
                continue
            pad_right = pad
            if causal and stride == 1:  # all the padding on the left
                pad, pad_right, t_out = (k - 1) * dil, 0, t
            if pad_mode == "reflect" and max(pad, pad_right) >= t:
                pad_mode = "replicate"  # (a reflection is shorter than the row)
        c.update(b=b, cin=cin, cout=cout, groups=groups, t=t, t_out=t_out, width=width, k=k, stride=stride, dil=dil,
                 pad=pad, pad_right=pad_right, out_pad=out_pad, pad_mode=pad_mode)
        c["wshape"] = (cin, cout // groups, k) if transposed else (cout, cin // groups, k)
        yield c


def epilogue_desc(c, backward=False):
    """Descriptor of a case; ``backward``: the one the gradient entry points take (zero padding, no epilogue terms)."""
    kw = dict(transposed=c["transposed"], width=c["width"], pre_act=c["pre_act"], pre_slope=c["pre_slope"])
    if not backward:
        kw.update(pad_mode=c["pad_mode"], post_act=c["post_act"], post_slope=c["post_slope"], out_mul=c["out_mul"],
                  out_div=c["out_div"])
    return ops.make_conv_desc(c["b"], c["cin"], c["cout"], c["t"], c["t_out"], c["k"], c["stride"], c["dil"], c["pad"],
                              c["groups"], **kw)


def _conv64(c, xa, w):
    if c["transposed"]:
        return F.conv_transpose1d(xa, w, None, stride=c["stride"], padding=c["pad"], output_padding=c["out_pad"],
                                  groups=c["groups"])
    if c["width"] > 1:
        y = F.conv2d(xa.reshape(c["b"], c["cin"], c["t"], c["width"]), w.unsqueeze(-1), None, stride=(c["stride"], 1),
                     padding=(c["pad"], 0))
        return y.flatten(2)
    xp = F.pad(xa, (c["pad"], c["pad_right"]), mode="constant" if c["pad_mode"] == "zero" else c["pad_mode"])
    return F.conv1d(xp, w, None, stride=c["stride"], dilation=c["dil"], groups=c["groups"])


def _out_at(shape, dev, off):
    """A NaN-filled destination (an element nobody writes fails the comparison), ``off`` floats off as above."""
    return _view_at(torch.full(shape, float("nan")), dev, off)


def run_epilogue(n_cases, seed):
    """Second sweep (``epilogue_cases``): forward with every drawn epilogue term, data gradient with mask and accum, and
    on a share of the cases the weight gradient under need_db=False and through the weight-norm finish, against float64
    on the CPU; addends, accum and outputs 4 bytes off a 16-byte boundary on a coin flip.  Pad-mode cases check the
    forward only (the gradients take zero padding only).  Returns (failing cases, number of cases that ran)."""
    dev = torch.device("cuda:0")
    bad, ran = [], 0
    for c in epilogue_cases(n_cases, seed):
        g = torch.Generator().manual_seed(10_000 + c["case"])
        b, cin, cout, wshape, off = c["b"], c["cin"], c["cout"], c["wshape"], c["off"]
        x = torch.randn(b, cin, c["t"] * c["width"], generator=g)
        x[torch.rand(x.shape, generator=g) < 0.05] = 0.0  # exact zeros: the mask edge of the data gradient
        w = torch.randn(wshape, generator=g) / ((cin // c["groups"]) * c["k"] / (c["stride"] if c["transposed"] else 1)) ** 0.5
        bias = torch.randn(cout, generator=g)
        oshape = (b, cout, c["t_out"] * c["width"])
        add1, add2, dy = (torch.randn(oshape, generator=g) for _ in range(3))
        accum = torch.randn(x.shape, generator=g)
        # float64 references
        x64, w64 = x.double().requires_grad_(), w.double().requires_grad_()
        pre = _conv64(c, _act64(x64, c["pre_act"], c["pre_slope"]), w64)
        assert tuple(pre.shape) == oshape, (tuple(pre.shape), oshape)
        s = pre.detach()
        if c["has_bias"]:
            s = s + bias.double().view(1, -1, 1)
        if c["has_add1"]:
            s = s + add1.double()
        if c["has_add2"]:
            s = s + add2.double()
        y_ref = _act64(s * c["out_mul"] / c["out_div"], c["post_act"], c["post_slope"])
        pre.backward(dy.double())
        dx_ref = x64.grad + accum.double()
        desc, desc_b = epilogue_desc(c), epilogue_desc(c, backward=True)
        xd, wd, bd, dyd = (v.to(dev).contiguous() for v in (x, w, bias, dy))
        a1d = _view_at(add1, dev, off) if c["has_add1"] else None
        a2d = _view_at(add2, dev, off) if c["has_add2"] else None
        tag = "case " + " ".join(f"{k2}={v}" for k2, v in c.items() if k2 != "wshape")
        errs = {}
        try:
            y = ops.conv1d_forward(desc, xd, ops.pack_weight(desc, wd), bd if c["has_bias"] else None, a1d, a2d,
                                   out=_out_at(oshape, dev, off))
            errs["y"] = rel(y, y_ref)
            if c["pad_mode"] == "zero":
                dx = ops.conv1d_backward_data(desc_b, dyd, ops.pack_weight_bwd(desc_b, wd), xd if c["pre_act"] else None,
                                              _view_at(accum, dev, off), out=_out_at(tuple(x.shape), dev, off))
                errs["dx"] = rel(dx, dx_ref)
            if c["pad_mode"] == "zero" and c["weight_grads"]:
                dw, none = ops.conv1d_backward_weight(desc_b, xd, dyd, wshape, need_db=False)
                assert none is None
                errs["dw"] = rel(dw, w64.grad)
                # weight-norm finish at g = ||v||, where the weight is v itself
                dv, dg, db = ops.conv1d_backward_weight_wn(desc_b, xd, dyd, wd, wd.flatten(1).norm(dim=1).contiguous())
                v64 = w.double().requires_grad_()
                g64 = wd.flatten(1).norm(dim=1).cpu().double().requires_grad_()
                wn = g64.view(-1, 1, 1) * v64 / v64.flatten(1).norm(dim=1).view(-1, 1, 1)
                (wn * w64.grad).sum().backward()
                errs.update(dv=rel(dv, v64.grad), dg=rel(dg.reshape(-1), g64.grad), db=rel(db, dy.double().sum(dim=(0, 2))))
        except RuntimeError as e:
            if "unsupported" in str(e).lower() or "dilation with stride" in str(e) or "status -2" in str(e):
                continue
            bad.append((tag, "exception " + str(e)[:120]))
            continue
        ran += 1
        if not (max(errs.values()) <= RTOL):
            bad.append((tag, {k2: f"{v:.2e}" for k2, v in errs.items()}))
    return bad, ran


def main():
    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    if len(sys.argv) > 3 and sys.argv[3] == "epilogue":
        bad, ran = run_epilogue(n_cases, seed)
        print(f"{n_cases} cases, {ran} ran, {len(bad)} failures")
    else:
        bad = run(n_cases, seed)
        print(f"{n_cases} cases, {len(bad)} failures")
    for t in bad[:30]:
        print("  FAIL", t)


if __name__ == "__main__":
    main()
