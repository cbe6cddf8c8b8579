"""GPU: the three data kernels of csrc/wavenet.hip (layer forward, gate backward, data backward) one by one against
the float64 references of tests/wavenet_refs.py, each on that kernel's OWN inputs, on a grid of sequence lengths and
dilations chosen for the kernels' edges:

  T = 1, 5 (below one float4 / one tile), 63, 64, 65 (tile - 1, exact, tile + 1), 100 (T % 4 == 0 on a ragged tile: the
  16-byte epilogues with their ``nq < T`` guard), 131 (odd: the scalar epilogues and the ragged tail), 196 (several
  32- and 64-column tiles); dilation 1 (taps inside), 3 (odd shift), 64 (= the tile width), 512 (larger than every T:
  both outer tap windows lie wholly outside the sequence).

What every launch has in common:

  * values within RTOL of float64, relative to the largest reference magnitude of the tensor;
  * stores: EVERY output of every launch here is a view in the middle of a buffer filled with a NaN-payload sentinel;
    after the launch the guard bands are bit-identical to the sentinel (a ragged tile wrote only its own elements; for
    ``dc``: the 80 aux rows and nothing behind row 79) and no output element still is the sentinel;
  * alignment (T = 100): a tensor that starts 4 bytes off a 16-byte boundary turns the 16-byte epilogue off
    (``vec_ok``), and the scalar epilogue must give the SAME BITS ("the arithmetic per element is unchanged");
  * one case of each kernel is launched twice: bit-identical.

The outputs are placed at chosen addresses by calling the C entry points directly (``_lib.lib()``)."""
import ctypes
import functools
import math

import pytest
import torch

from parallelwavegan_amd import _lib, ops
from parallelwavegan_amd.layers.residual_block import WaveNetResidualBlock
from tests import wavenet_refs as R
from tests.elementwise_refs import f32
from tests.util import poison_empty, poison_lds

pytestmark = pytest.mark.gpu

# The project's fp32 bar for this kernel, relative to the largest reference magnitude (RTOL of
# tests/test_wavenet_layer_gpu.py::test_layer_kernel_matches_aten); the longest reduction here is 384 products.  The
# float32 CPU evaluation of the same formulas stays within 1e-6 of float64 over this grid, so the data leave the bar
# about 30x of room.
RTOL = 3e-5
# g = tanh * sigmoid on hardware exp2 / rcp: |g| <= 1, so this absolute bound is RTOL's order relative to the maximum
# while not being diluted by saturated rows (csrc/wavenet_gate.h states ~1e-7 for O(1) arguments; the argument
# -z * log2(e) is rounded to fp32, 1e-6 absolute at |z| ~ 20)
GATE_ATOL = 3e-6
# quantities that pass through two or three kernels (tests/test_wavenet_layer_gpu.py::test_fused_layer_autograd_matches_unfused)
LAYER_RTOL = 5e-5
GUARD = 64             # floats of guard band on each side of an output view (256 B: keeps the view 16-B aligned)
SENTINEL = 0x7FC5A5A5  # a quiet NaN with a payload no kernel produces
AUX = 80
OUT_MUL, SKIP_MUL = math.sqrt(0.5), math.sqrt(1 / 30)

TS = (1, 5, 63, 64, 65, 100, 131, 196)
DILS = (1, 3, 64, 512)
GRID = [(T, dil) for T in TS for dil in DILS]
GRID_IDS = [f"T{T}-d{dil}" for T, dil in GRID]
VARIANT_TS = (5, 100, 131)  # the variants run at dilation 3
TWICE = (131, 3)            # the case that is launched twice

# entry point of csrc/wavenet.hip -> the test that drives it directly (checked by tests/test_wavenet_refs_host.py)
COVERED = {
    "pwg_wavenet_layer_supported": "test_forward",
    "pwg_wavenet_packed_weight_floats": "test_forward",
    "pwg_wavenet_pack_weights": "test_backward_image",
    "pwg_wavenet_layer_forward": "test_forward",
    "pwg_wavenet_packed_weight_bwd_floats": "test_gate_backward",
    "pwg_wavenet_pack_weights_bwd": "test_backward_image",
    "pwg_wavenet_gate_backward": "test_gate_backward",
    "pwg_wavenet_data_backward": "test_data_backward",
    # the weight path has a matrix of its own: ``module::test``
    "pwg_wavenet_weight_backward_workspace_floats": "tests.test_wavenet_wgrad_matrix_gpu::test_edge_grid",
    "pwg_wavenet_weight_backward_plan": "tests.test_wavenet_wgrad_matrix_gpu::test_finish_exact_long",
    "pwg_wavenet_weight_backward": "tests.test_wavenet_wgrad_matrix_gpu::test_edge_grid",
}


# ------------------------------------------------------------------------------------------------ inputs, shared
@functools.lru_cache(maxsize=None)
def _weights():
    """CPU float32 weights, biases and four distinct row scales (read-only, shared by every test)."""
    g = torch.Generator().manual_seed(2024)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    ru = lambda n: torch.rand(n, generator=g)  # noqa: E731
    return dict(w_d=rn(128, 64, 3) / math.sqrt(192), w_a=rn(128, AUX, 1) / math.sqrt(AUX), w_s=rn(64, 64, 1) / 8,
                w_o=rn(64, 64, 1) / 8, b_d=rn(128), b_s=rn(64), b_o=rn(64),
                s_d=1.0 + 0.2 * ru(128), s_a=0.7 + 0.2 * ru(128), s_s=1.3 + 0.2 * ru(64), s_o=0.5 + 0.2 * ru(64))


@functools.lru_cache(maxsize=None)
def _data(B, T):
    """CPU float32 operands of every kernel at (B, T): each kernel gets inputs of its own, not another kernel's result."""
    g = torch.Generator().manual_seed(7919 * B + T)
    shapes = dict(x=64, c=AUX, skips=64, z=128, dx_out=64, ds_out=64, dz=128, go=64, dc_accum=AUX)
    return {n: torch.randn(B, ch, T, generator=g) for n, ch in shapes.items()}


@functools.lru_cache(maxsize=None)
def _eff(scaled=True):
    """(Wd, Wa, Ws, Wo): the effective weights in float64."""
    w = _weights()
    return tuple(R.effective(w["w_" + n], w["s_" + n] if scaled else None) for n in "daso")


@functools.lru_cache(maxsize=None)
def _z_ref(B, T, dil, bias, scaled):
    w, t = _weights(), _data(B, T)
    Wd, Wa, Ws, Wo = _eff(scaled)
    return R.layer_forward(t["x"].double(), t["c"].double(), None, Wd, Wa, Ws, Wo, w["b_d"].double() if bias else None,
                           None, None, dil, 1.0, 1.0)[0]


class Guarded:
    """An output view of ``shape`` in the middle of a sentinel-filled buffer, ``off`` floats past a 16-byte boundary."""

    def __init__(self, shape, device, off=0):
        n = math.prod(shape)
        self.buf = torch.full((GUARD + off + n + GUARD,), SENTINEL, dtype=torch.int32, device=device)
        self.lo, self.hi = GUARD + off, GUARD + off + n
        self.out = self.buf[self.lo:self.hi].view(torch.float32).view(shape)
        assert self.out.data_ptr() % 16 == 4 * off

    def check(self, what):
        assert bool((self.buf[:self.lo] == SENTINEL).all()), f"{what}: store below the output"
        assert bool((self.buf[self.hi:] == SENTINEL).all()), f"{what}: store past the output"
        left = int((self.buf[self.lo:self.hi] == SENTINEL).sum())
        assert left == 0, f"{what}: {left} output elements never written"
        return self.out


def _off4(t):
    """A copy of ``t`` that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _place(t, device, off):
    """``t`` on the device, 16-byte aligned or (``off``) 4 bytes past such a boundary."""
    t = t.to(device)
    assert t.data_ptr() % 16 == 0
    return _off4(t) if off else t


def _call(name, desc, *tensors):
    lib = _lib.lib()
    rc = getattr(lib, name)(ctypes.byref(desc), *[ops._ptr(t) for t in tensors], ops._stream())
    assert rc == 0, f"{name}: status {rc}: {lib.pwg_last_error().decode(errors='replace')}"


def _err(got, want):
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    return (got - want).abs().max().item() / (want.abs().max().item() + 1e-12)


def _within(got, want, what, tol=RTOL):
    assert torch.isfinite(got).all(), f"{what}: not finite"
    err = _err(got, want)
    print(f"{what}: rel-to-max error {err:.3e}")
    assert err <= tol, f"{what}: rel-to-max error {err:.3e}"


def _same_bits(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k}: {int((a[k] != b[k]).sum())} values differ"


def _images(device, desc, scaled=True, weights=None, bwd=False):
    w = weights or _weights()
    args = []
    for n in "daso":
        args += [w["w_" + n].to(device), w["s_" + n].to(device) if scaled else None]
    return (ops.wavenet_pack_weights_bwd if bwd else ops.wavenet_pack_weights)(desc, *args)


# ------------------------------------------------------------------------------------------------ forward
def _run_forward(device, B, T, dil, save=True, bias=True, scaled=True, skips=True, muls=(OUT_MUL, SKIP_MUL), inplace=False,
                 off=None, b_d=None, img=None):
    """One launch of the layer kernel -> {name: tensor} of its outputs, every one of them from a guarded buffer.
    ``off``: the name of the operand or output that starts 4 bytes off a 16-byte boundary."""
    w, t = _weights(), _data(B, T)
    desc = ops.make_wavenet_desc(B, T, dil, out_mul=muls[0], skip_mul=muls[1])
    assert ops.wavenet_layer_supported(desc)
    what = f"forward B{B} T{T} d{dil} off={off}"
    with poison_lds(), poison_empty():
        if img is None:
            img = _images(device, desc, scaled)
        x, c = _place(t["x"], device, off == "x"), _place(t["c"], device, off == "c")
        sk = _place(t["skips"], device, off == "skips") if skips else None
        names = ("x_out", "skips_out") + (("z", "g") if save else ())
        gd = {n: Guarded((B, 128 if n == "z" else 64, T), device, int(off == n)) for n in names}
        if inplace:  # the running skip sum is accumulated where it lies
            gd["skips_out"].out.copy_(sk)
            sk = gd["skips_out"].out
        b_d = (w["b_d"] if b_d is None else b_d).to(device) if bias else None
        b_s, b_o = (w["b_s"].to(device), w["b_o"].to(device)) if bias else (None, None)
        _call("pwg_wavenet_layer_forward", desc, x, c, sk, img, b_d, b_s, b_o, gd["x_out"].out, gd["skips_out"].out,
              gd["z"].out if save else None, gd["g"].out if save else None)
        return {n: gd[n].check(f"{what}: {n}") for n in names}


def _check_forward(out, B, T, dil, bias=True, scaled=True, skips=True, muls=(OUT_MUL, SKIP_MUL), what=""):
    """z against float64; g on the kernel's own z; the two outputs on the kernel's own g."""
    w, t = _weights(), _data(B, T)
    _, _, Ws, Wo = _eff(scaled)
    b_s, b_o = (w["b_s"].double(), w["b_o"].double()) if bias else (None, None)
    _within(out["z"], _z_ref(B, T, dil, bias, scaled), what + " z")
    _within(out["g"], R.gate(out["z"].cpu().double()), what + " g")
    kg = out["g"].cpu().double()
    _within(out["skips_out"], R.skip_out(kg, t["skips"].double() if skips else None, Ws, b_s, f32(muls[1])), what + " skips_out")
    _within(out["x_out"], R.res_out(kg, t["x"].double(), Wo, b_o, f32(muls[0])), what + " x_out")


@pytest.mark.parametrize("T,dil", GRID, ids=GRID_IDS)
def test_forward(T, dil, device):
    B = 2
    out = _run_forward(device, B, T, dil)
    _check_forward(out, B, T, dil, what="grid")
    if (T, dil) == TWICE:
        _same_bits(out, _run_forward(device, B, T, dil), "second launch")
    if dil != 3 or T not in VARIANT_TS:
        return
    # inference form: z and g are not written; same bits
    lean = _run_forward(device, B, T, dil, save=False)
    assert set(lean) == {"x_out", "skips_out"}
    _same_bits(lean, out, "save=False")
    # the running skip sum accumulated in place: same bits
    _same_bits(_run_forward(device, B, T, dil, inplace=True), out, "skips_out is skips")
    for kw in (dict(bias=False), dict(scaled=False), dict(skips=False), dict(muls=(1.0, 1.0))):
        _check_forward(_run_forward(device, B, T, dil, **kw), B, T, dil, what=str(kw), **kw)
    _check_forward(_run_forward(device, 3, T, dil), 3, T, dil, what="B=3")


@pytest.mark.parametrize("dil", [3, 512])
@pytest.mark.parametrize("T", VARIANT_TS)
def test_forward_stores(T, dil, device):
    """x_out, skips_out, z and g in guarded buffers (``Guarded.check`` inside ``_run_forward``): bands intact, every
    element written -- with and without the running skip sum, whose absence changes no store."""
    for skips in (True, False):
        out = _run_forward(device, 2, T, dil, skips=skips)
        assert set(out) == {"x_out", "skips_out", "z", "g"}
        assert all(torch.isfinite(v).all() for v in out.values())


def test_forward_alignment(device):
    """T = 100 (T % 4 == 0: the aligned launch takes the 16-byte epilogue).  ``skips``, ``skips_out``, ``x_out``, ``z``
    and ``g`` in turn 4 bytes off a 16-byte boundary: the scalar epilogue, the same bits.  x and c 4 bytes off change
    the operand DMA (not the epilogue): the values stay within the bar."""
    B, T, dil = 2, 100, 3
    base = _run_forward(device, B, T, dil)
    _check_forward(base, B, T, dil, what="aligned")
    for off in ("skips", "skips_out", "x_out", "z", "g"):
        _same_bits(_run_forward(device, B, T, dil, off=off), base, f"{off} 4 bytes off")
    for off in ("x", "c"):
        _check_forward(_run_forward(device, B, T, dil, off=off), B, T, dil, what=f"{off} 4 bytes off")


SATURATED = (20.0, -20.0, 90.0, -90.0, 1e4, -1e4)


def test_forward_saturation(device):
    """Rows of b_dil at +-20, +-90 and +-1e4 on the tanh half, on the sigmoid half, and on both halves of one channel:
    ``gate_fast`` relies on 2^inf = inf -> rcp = 0."""
    B, T, dil = 2, 65, 3
    w, t = _weights(), _data(B, T)
    b_d = w["b_d"].clone()
    for i, v in enumerate(SATURATED):
        b_d[i] = v            # tanh half of channel i
        b_d[64 + 8 + i] = v   # sigmoid half of channel 8 + i
        b_d[16 + i], b_d[64 + 16 + i] = v, SATURATED[(i + 3) % 6]  # both halves of channel 16 + i
    out = _run_forward(device, B, T, dil, b_d=b_d)
    for n, v in out.items():
        assert torch.isfinite(v).all(), n
    g_ref = R.gate(out["z"].cpu().double())
    err = (out["g"].cpu().double() - g_ref).abs().max().item()
    print(f"g: max abs error {err:.3e}")
    assert err <= GATE_ATOL, err
    assert float(out["g"].abs().max()) <= 1.0
    _, _, Ws, Wo = _eff()
    kg = out["g"].cpu().double()
    _within(out["skips_out"], R.skip_out(kg, t["skips"].double(), Ws, w["b_s"].double(), f32(SKIP_MUL)), "skips_out")
    _within(out["x_out"], R.res_out(kg, t["x"].double(), Wo, w["b_o"].double(), f32(OUT_MUL)), "x_out")


# ------------------------------------------------------------------------------------------------ gate backward
def _run_gate(device, B, T, dil, with_dx=True, muls=(OUT_MUL, SKIP_MUL), off=None, z=None, img=None):
    t = _data(B, T)
    desc = ops.make_wavenet_desc(B, T, dil, out_mul=muls[0], skip_mul=muls[1])
    what = f"gate backward B{B} T{T} d{dil} off={off}"
    with poison_lds(), poison_empty():
        if img is None:
            img = _images(device, desc, bwd=True)
        zd = _place(t["z"] if z is None else z, device, off == "z")
        dx_out = t["dx_out"].to(device) if with_dx else None
        gd = {"dz": Guarded((B, 128, T), device, int(off == "dz"))}
        if with_dx:
            gd["go"] = Guarded((B, 64, T), device, int(off == "go"))
        _call("pwg_wavenet_gate_backward", desc, zd, dx_out, t["ds_out"].to(device), img, gd["dz"].out,
              gd["go"].out if with_dx else None)
        return {n: g.check(f"{what}: {n}") for n, g in gd.items()}


def _check_gate(out, B, T, with_dx=True, muls=(OUT_MUL, SKIP_MUL), z=None, what=""):
    t = _data(B, T)
    _, _, Ws, Wo = _eff()
    dz, go = R.gate_backward((t["z"] if z is None else z).double(), t["dx_out"].double() if with_dx else None,
                             t["ds_out"].double(), Ws, Wo, f32(muls[0]), f32(muls[1]))
    _within(out["dz"], dz, what + " dz")
    assert (go is None) == ("go" not in out)
    if go is not None:
        _within(out["go"], go, what + " go")


@pytest.mark.parametrize("T,dil", GRID, ids=GRID_IDS)
def test_gate_backward(T, dil, device):
    B = 2
    out = _run_gate(device, B, T, dil)
    _check_gate(out, B, T, what="grid")
    if (T, dil) == TWICE:
        _same_bits(out, _run_gate(device, B, T, dil), "second launch")
    if dil != 3 or T not in VARIANT_TS:
        return
    # the last layer: no residual gradient, no go, dz from the skip path alone
    alone = _run_gate(device, B, T, dil, with_dx=False)
    assert set(alone) == {"dz"}
    _check_gate(alone, B, T, with_dx=False, what="dx_out=None")
    _check_gate(_run_gate(device, B, T, dil, muls=(1.0, 1.0)), B, T, muls=(1.0, 1.0), what="muls=1")
    _check_gate(_run_gate(device, 3, T, dil), 3, T, what="B=3")
    if T != 100:
        return
    # T % 4 == 0: z, dz and go in turn 4 bytes off a 16-byte boundary -> the scalar path, the same bits
    for off in ("z", "dz", "go"):
        _same_bits(_run_gate(device, B, T, dil, off=off), out, f"{off} 4 bytes off")
    # saturated gate inputs: exp2 overflows to inf, rcp(inf) = 0, no inf * 0
    z = _data(B, T)["z"].clone()
    flat, g = z.view(-1), torch.Generator().manual_seed(5)
    idx = torch.randperm(flat.numel(), generator=g)[:600]
    flat[idx] = torch.tensor(SATURATED).repeat(100)
    sat = _run_gate(device, B, T, dil, z=z)
    _check_gate(sat, B, T, z=z, what="saturated z")


# ------------------------------------------------------------------------------------------------ data backward
def _run_data(device, B, T, dil, with_go=True, need_dx=True, need_dc=True, accum=None, img=None):
    """``accum``: None, "given" (a tensor of its own) or "alias" (``dc`` itself holds the accumulated gradient)."""
    t = _data(B, T)
    desc = ops.make_wavenet_desc(B, T, dil, out_mul=OUT_MUL, skip_mul=SKIP_MUL)
    what = f"data backward B{B} T{T} d{dil}"
    with poison_lds(), poison_empty():
        if img is None:
            img = _images(device, desc, bwd=True)
        gd = {}
        if need_dx:
            gd["dx"] = Guarded((B, 64, T), device)
        if need_dc:
            gd["dc"] = Guarded((B, AUX, T), device)
        acc = None
        if accum == "given":
            acc = t["dc_accum"].to(device)
        elif accum == "alias":
            gd["dc"].out.copy_(t["dc_accum"])
            acc = gd["dc"].out
        _call("pwg_wavenet_data_backward", desc, t["dz"].to(device), t["go"].to(device) if with_go else None, img, acc,
              gd["dx"].out if need_dx else None, gd["dc"].out if need_dc else None)
        return {n: g.check(f"{what}: {n}") for n, g in gd.items()}


def _check_data(out, B, T, dil, with_go=True, accum=None, what=""):
    t = _data(B, T)
    Wd, Wa, _, _ = _eff()
    dx, dc = R.data_backward(t["dz"].double(), t["go"].double() if with_go else None, Wd, Wa, dil,
                             t["dc_accum"].double() if accum else None)
    if "dx" in out:
        _within(out["dx"], dx, what + " dx")
    if "dc" in out:
        _within(out["dc"], dc, what + " dc")


# (T = 33: one full 32-column tile of the data-gradient kernel and a tile of one column)
@pytest.mark.parametrize("T,dil", GRID + [(33, 3), (33, 512)], ids=GRID_IDS + ["T33-d3", "T33-d512"])
def test_data_backward(T, dil, device):
    B = 2
    out = _run_data(device, B, T, dil)
    assert set(out) == {"dx", "dc"}
    _check_data(out, B, T, dil, what="grid")
    if (T, dil) == TWICE:
        _same_bits(out, _run_data(device, B, T, dil), "second launch")
    if dil != 3 or T not in VARIANT_TS + (33,):
        return
    _check_data(_run_data(device, B, T, dil, with_go=False), B, T, dil, with_go=False, what="go=None")
    only_dc = _run_data(device, B, T, dil, need_dx=False)
    assert set(only_dc) == {"dc"} and torch.equal(only_dc["dc"], out["dc"])
    only_dx = _run_data(device, B, T, dil, need_dc=False)
    assert set(only_dx) == {"dx"} and torch.equal(only_dx["dx"], out["dx"])
    given = _run_data(device, B, T, dil, accum="given")
    _check_data(given, B, T, dil, accum="given", what="dc_accum")
    # dc_accum may be dc itself: every element is read and written by the same lane
    _same_bits(_run_data(device, B, T, dil, accum="alias"), given, "dc_accum is dc")
    _check_data(_run_data(device, 3, T, dil, accum="given", need_dx=False), 3, T, dil, accum="given", what="B=3")


# ------------------------------------------------------------------------------------------------ weight images
def test_backward_image(device):
    """``pwg_wavenet_pack_weights`` and ``pwg_wavenet_pack_weights_bwd`` through their results: the three data kernels on
    an image packed from (w, scale) -- and, backward, with out_mul / skip_mul folded by the packer -- give THE SAME BITS
    as on an image packed from the pre-multiplied float32 weights with scale None and multipliers 1.  Exact equality
    (not one ulp) holds because both packers form ``(w * scale) * mul`` left to right, every product rounded once to
    float32 and never next to an addition it could be contracted with, and ``* 1.f`` is exact."""
    B, T, dil = 2, 100, 3
    w = _weights()
    pre = dict(w)
    for n in "daso":
        pre["w_" + n] = w["w_" + n] * w["s_" + n].view(-1, 1, 1)  # float32 product, rounded once
    desc = ops.make_wavenet_desc(B, T, dil, out_mul=OUT_MUL, skip_mul=SKIP_MUL)
    unit = ops.make_wavenet_desc(B, T, dil, out_mul=1.0, skip_mul=1.0)
    with poison_lds(), poison_empty():
        img_pre = _images(device, desc, scaled=False, weights=pre)
    _same_bits(_run_forward(device, B, T, dil, img=img_pre), _run_forward(device, B, T, dil), "forward image")
    folded = dict(pre)
    folded["w_s"] = pre["w_s"] * torch.tensor(SKIP_MUL, dtype=torch.float32)
    folded["w_o"] = pre["w_o"] * torch.tensor(OUT_MUL, dtype=torch.float32)
    with poison_lds(), poison_empty():
        img_folded = _images(device, unit, scaled=False, weights=folded, bwd=True)
    gate = _run_gate(device, B, T, dil)
    _check_gate(gate, B, T, what="(w, scale) image")
    _same_bits(_run_gate(device, B, T, dil, img=img_folded), gate, "gate image")
    data = _run_data(device, B, T, dil)
    _check_data(data, B, T, dil, what="(w, scale) image")
    _same_bits(_run_data(device, B, T, dil, img=img_folded), data, "dx / dc image")


# ------------------------------------------------------------------------------------------------ the layer, end to end
LAYER_SHAPES = [(2, 77, 4), (1, 3, 1), (2, 130, 512)]
# with_skips, skip_scale, residual output used
LAYER_MODES = [(False, 1.0, True), (True, 1.0, True), (False, SKIP_MUL, True), (True, SKIP_MUL, True), (True, SKIP_MUL, False)]


@pytest.mark.parametrize("with_skips,skip_scale,use_res", LAYER_MODES)
@pytest.mark.parametrize("B,T,dil", LAYER_SHAPES)
def test_layer_autograd_matches_float64(B, T, dil, with_skips, skip_scale, use_res, device):
    """``WaveNetResidualBlock`` (weight norm, one-launch layer) against torch autograd in float64 on the CPU, on the
    reference formula with the block's parameters copied over: outputs, dx, dc, ds and every parameter gradient.  T is
    no multiple of 4, and the reference is not this project's own GPU code."""
    torch.manual_seed(100 * T + dil)
    blk = WaveNetResidualBlock(dilation=dil)
    for cv in blk.fused_convs():
        cv.apply_weight_norm()
    with torch.no_grad():
        for p in blk.parameters():
            p.add_(0.05 * torch.randn_like(p))
    x0, c0, s0 = torch.randn(B, 64, T), torch.randn(B, AUX, T), torch.randn(B, 64, T)
    wx, ws = torch.randn(B, 64, T), torch.randn(B, 64, T)
    # float64 on the CPU
    p64 = {n: p.detach().double().requires_grad_() for n, p in blk.named_parameters()}

    def weight(name):
        v, g = p64[name + ".weight_v"], p64[name + ".weight_g"]
        return g * v / v.flatten(1).norm(dim=1).view(-1, 1, 1)

    x, c = x0.double().requires_grad_(), c0.double().requires_grad_()
    s = s0.double().requires_grad_() if with_skips else None
    _, _, so, xo = R.layer_forward(x, c, s, weight("conv"), weight("conv1x1_aux"), weight("conv1x1_skip"),
                                   weight("conv1x1_out"), p64["conv.bias"], p64["conv1x1_skip.bias"],
                                   p64["conv1x1_out.bias"], dil, f32(math.sqrt(0.5)), f32(skip_scale))
    loss = (so * ws.double()).sum() + ((xo * wx.double()).sum() if use_res else 0.0)
    leaves = dict(dx=x, dc=c, **p64)
    if with_skips:
        leaves["ds"] = s
    grads = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    want = dict(zip(leaves, grads), xo=xo.detach(), so=so.detach())
    # the block on the GPU
    blk = blk.to(device)
    blk.fuse_layer = True
    xg, cg = x0.to(device).requires_grad_(), c0.to(device).requires_grad_()
    sg = s0.to(device).requires_grad_() if with_skips else None
    with poison_lds(), poison_empty():
        xo_g, so_g = blk(xg, cg, skips=sg, skip_scale=skip_scale)
        assert "WaveNetLayerFn" in type(so_g.grad_fn).__name__, type(so_g.grad_fn).__name__
        loss_g = (so_g * ws.to(device)).sum() + ((xo_g * wx.to(device)).sum() if use_res else 0.0)
        loss_g.backward()
    got = dict(xo=xo_g.detach(), so=so_g.detach(), dx=xg.grad, dc=cg.grad, **{n: p.grad for n, p in blk.named_parameters()})
    if with_skips:
        got["ds"] = sg.grad
    assert set(got) == set(want)
    for k, ref in want.items():
        if ref is None or float(ref.abs().max()) == 0.0:  # the residual 1x1 of a layer whose residual output is unused
            assert not use_res and k.startswith("conv1x1_out"), k
            assert got[k] is None or float(got[k].abs().max()) == 0.0, k
            continue
        assert got[k] is not None, k
        _within(got[k], ref, k, LAYER_RTOL)
