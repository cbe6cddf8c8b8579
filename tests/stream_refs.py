"""References of the conv stream launch (csrc/conv1d_stream.hip, csrc/stream_common.h), one function per rule, written
from the definitions in the two files' header comments in plain CPU torch.  Every function computes in the dtype of its
tensor arguments: float64 is the reference of tests/test_conv_stream_matrix_gpu.py, float32 the measurement of how
much of the bar the arithmetic itself uses (tests/test_stream_refs_host.py).  The rules that only move data (history,
window, delay line) return bit-exact copies in any dtype.

Shapes: x (B, C_in, n) the chunk; hist (B, C_in, H) the raw history; a window (B, C_in, H + n), column H + t of which is
chunk-relative column t; w in torch layout, (C_out, C_in, k) or, transposed, (C_in, C_out, 2 s)."""
import torch

from tests.elementwise_refs import f32


# ------------------------------------------------------------------------------------------------ history rule
def history(hist_in, x, H, replicate=False):
    """hist_out: the last H raw columns of concat(hist_in, x), also for n < H.  ``hist_in`` None is the start of a
    stream: zeros, or the replicated first column under replicate padding."""
    B, C, n = x.shape
    if hist_in is None:
        hist_in = x[..., :1].expand(B, C, H) if replicate else x.new_zeros(B, C, H)
    assert hist_in.shape == (B, C, H), (hist_in.shape, (B, C, H))
    return torch.cat([hist_in, x], -1)[..., n:].clone()


# ------------------------------------------------------------------------------------------------ start-of-stream rule
def window(hist_in, x, H, pad_mode="zero", transposed=False):
    """The H + n raw columns a chunk is computed from: the history, or at the start of a stream (``hist_in`` None) what
    ``pad_mode`` synthesises -- zero: nothing; replicate: x[0]; reflect: column -j is x[j] (stride-1 form only)."""
    B, C, n = x.shape
    if hist_in is not None:
        left = hist_in
    elif pad_mode == "zero":
        left = x.new_zeros(B, C, H)
    elif pad_mode == "replicate":
        left = x[..., :1].expand(B, C, H)
    else:
        assert pad_mode == "reflect" and not transposed and n > H, (pad_mode, transposed, n, H)
        left = x[..., 1:H + 1].flip(-1)
    assert left.shape == (B, C, H)
    return torch.cat([left, x], -1)


# ------------------------------------------------------------------------------------------------ activations, epilogue
def act(v, kind=None, slope=0.0):
    if kind in (None, "none"):
        return v
    if kind == "leaky_relu":
        return torch.where(v > 0, v, v * f32(slope))
    if kind == "relu":
        return torch.where(v > 0, v, torch.zeros_like(v))
    assert kind == "tanh", kind
    return torch.tanh(v)


def epilogue(v, bias=None, add1=None, add2=None, out_mul=1.0, out_div=1.0, post_act=None, post_slope=0.0):
    """bias, add1, add2, out_mul, out_div, post-activation, in that order (out_mul / out_div as the float32 values the
    descriptor carries)."""
    if bias is not None:
        v = v + bias.view(1, -1, 1)
    if add1 is not None:
        v = v + add1
    if add2 is not None:
        v = v + add2
    if out_mul != 1.0:
        v = v * f32(out_mul)
    if out_div != 1.0:
        v = v / f32(out_div)
    return act(v, post_act, post_slope)


# ------------------------------------------------------------------------------------------------ plain chunk, stride 1
def contract(win, w, dil, pre_act=None, pre_slope=0.0):
    """Y[m][j] = sum_{tap, ci} W[m][ci][tap] * act(X[ci][j - H + tap * dil]), H = (k - 1) * dil; the pre-activation is
    applied to history and chunk alike."""
    k = w.shape[-1]
    n = win.shape[-1] - (k - 1) * dil
    assert n > 0
    a = act(win, pre_act, pre_slope)
    y = 0
    for tap in range(k):
        y = y + torch.einsum("oc,bct->bot", w[:, :, tap], a[..., tap * dil:tap * dil + n])
    return y


def conv_chunk(win, w, dil, pre_act=None, pre_slope=0.0, **epi):
    return epilogue(contract(win, w, dil, pre_act, pre_slope), **epi)


# ------------------------------------------------------------------------------------------------ plain chunk, transposed
def contract_transposed(win, w, s, pre_act=None, pre_slope=0.0):
    """k = 2 s polyphase: output column j * s + phase = sum_ci x[ci][j - 1] * w[ci][co][phase + s] + x[ci][j] *
    w[ci][co][phase]; ``win`` holds one history column."""
    assert w.shape[-1] == 2 * s
    a = act(win, pre_act, pre_slope)
    prev, cur = a[..., :-1], a[..., 1:]
    y = torch.einsum("bcj,cop->bojp", prev, w[:, :, s:]) + torch.einsum("bcj,cop->bojp", cur, w[:, :, :s])
    return y.reshape(y.shape[0], y.shape[1], -1)


def transposed_chunk(win, w, s, pre_act=None, pre_slope=0.0, **epi):
    return epilogue(contract_transposed(win, w, s, pre_act, pre_slope), **epi)


# ------------------------------------------------------------------------------------------------ delayed form
def delayed_addend(line_in, add, delay):
    """What output column j adds: concat(line_in, add)[j]; ``line_in`` None reads as zeros."""
    if add is None:
        return None
    B, C, t_out = add.shape
    if line_in is None:
        line_in = add.new_zeros(B, C, delay)
    assert line_in.shape == (B, C, delay)
    return torch.cat([line_in, add], -1)[..., :t_out]


def line_out(line_in, add, delay):
    """The delay line a launch leaves: the history rule on (c_out, t_out) rows, zero start."""
    return history(line_in, add, delay)


def zero_outside(y, valid_lo, valid_hi):
    """Output columns outside [valid_lo, valid_hi) are exact zeros."""
    out = torch.zeros_like(y)
    lo, hi = max(valid_lo, 0), min(valid_hi, y.shape[-1])
    if hi > lo:
        out[..., lo:hi] = y[..., lo:hi]
    return out


def delayed_chunk(acc, valid, add1=None, line1=None, delay1=0, add2=None, line2=None, delay2=0, **epi):
    """``acc``: the contraction of the chunk (contract / contract_transposed).  The epilogue with both addends read
    through their delay lines, zeros outside ``valid``."""
    y = epilogue(acc, add1=delayed_addend(line1, add1, delay1), add2=delayed_addend(line2, add2, delay2), **epi)
    return zero_outside(y, *valid)


# ------------------------------------------------------------------------------------------------ window rule
def slot_window(delay, rate, t_out, before, left, left_known):
    """stream_slot_window: [max(delay - before * rate, 0), delay + left * rate), clamped to [0, t_out]; the upper edge is
    t_out while ``left`` is not known."""
    clamp = lambda v: max(0, min(t_out, v))  # noqa: E731
    return clamp(delay - before * rate), clamp(delay + left * rate if left_known else t_out)


# ------------------------------------------------------------------------------------------------ mirror rule
def mirror_column(t, in_lo, in_hi):
    """StreamMirrorWindow::at, first step: the column reflection reads for window column t (``in_hi`` None: not known)."""
    if t < in_lo:
        return 2 * in_lo - t
    if in_hi is not None and t >= in_hi:
        return 2 * (in_hi - 1) - t
    return t


def mirror_window(hist_in, x, H, in_lo, in_hi):
    """The window of the mirrored form: column t reads raw column mirror_column(t) of concat(hist_in, x) (zeros for a
    NULL history), and zero where that lies outside [-H, n)."""
    raw = window(hist_in, x, H, "zero")
    n = x.shape[-1]
    win = torch.zeros_like(raw)
    for t in range(-H, n):
        m = mirror_column(t, in_lo, in_hi)
        if -H <= m < n:
            win[..., H + t] = raw[..., H + m]
    return win
