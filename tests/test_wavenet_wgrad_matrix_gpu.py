"""GPU: the weight path of csrc/wavenet.hip -- ``wavenet_wgrad_kernel<272>``, ``wavenet_wgrad_kernel<64>``,
``wavenet_wgrad_finish_kernel`` and the slicing rule -- slice by slice against the float64 references of
tests/wavenet_refs.py, in the form tests/test_wavenet_matrix_gpu.py gives the three data kernels.

Every launch is a direct call of ``pwg_wavenet_weight_backward`` (``_lib.lib()``), so that every buffer sits at a chosen
address: each output asked for (dw / dg / db of the four convolutions) and the workspace are views in the middle of
sentinel-filled buffers; after the call the guard bands are bit-identical to the sentinel and no element of an output or
of the workspace still is the sentinel.  The workspace view is exactly ``workspace_floats`` long (the last slab ends on
its last float) and is read back: the slabs ``[slices][128][N + 1]`` are compared one by one with
``R.weight_backward_slabs``, so a wrong chunk is named by launch, slice, row and column.

  a. edge grid: T around the float4, the 32-column chunk and its multiples x dilations of every residue mod 4, smaller
     than, equal to and larger than a chunk and than every T (guarded and interior loads, the left-edge patterns);
  b. the finish, exactly: final values against the float64 sum of the float32 slabs read back, within a bound of counted
     roundings, over slice counts on both sides of every multiple of the 4-way unrolled walk of 3 and of 12 slice lanes;
  c. slicing: one chunk in total, one chunk per item, slices that straddle items, an odd chunk at the end of the range;
  d. variants: optional outputs, weight norm per convolution, operands off a 16-byte boundary, a dirty workspace;
  e. refusals: the error code of every PWG_REQUIRE line, and that no output byte changes;
  f. the layer: the operands ``WaveNetLayerFn`` hands the kernel are the ones the references assume.

Bars.  RTOL = 2e-5 relative to the largest reference magnitude is the bar tests/test_wavenet_layer_gpu.py already holds
this kernel to; the float32 CPU evaluation of the same contractions stays within 7.0e-7 of float64 over grids (a) and
(c) (tests/test_wavenet_refs_host.py::test_float32_room_and_sensitivity), so the data leave the bar about 29x of room.
Measured on an MI355X (worst over all cases): final outputs 3.7e-7 and slabs 4.5e-7 (0.019 and 0.022 of the bar), weight
norm 2.8e-7 (0.014 of the bar), the finish 0.32 of its counted bound; the whole file runs in 5.4 s."""
import ctypes
import functools

import pytest
import torch

from parallelwavegan_amd import _lib, ops
from tests import test_wavenet_matrix_gpu as M
from tests import wavenet_refs as R
from tests.util import poison_empty, poison_lds

pytestmark = pytest.mark.gpu

RTOL = 2e-5  # tests/test_wavenet_layer_gpu.py::test_weight_backward_kernel_matches_float64
AUX = 80
N0, N1 = 3 * 64 + AUX, 64  # columns of the two contractions; a slab row has one more (the row sum)
U = 2.0 ** -24             # unit roundoff of float32
SL = (3, 12)               # slice lanes of the finish kernel per launch
CONVS = ("dil", "aux", "skip", "out")
SHAPES = dict(dil=(128, 64, 3), aux=(128, AUX, 1), skip=(64, 64, 1), out=(64, 64, 1))
OPERANDS = ("dz", "x", "c", "gs", "go", "g")
ROWS = dict(dz=128, x=64, c=AUX, gs=64, go=64, g=64)
BIASES = ("dil", "skip", "out")  # the layer's convolutions that have a bias (conv1x1_aux has none)
# output of a launch -> key of R.weight_backward (db of the aux convolution, if asked for, is db of the dilated one)
REF_KEY = dict(dw_dil="dWd", dw_aux="dWa", dw_skip="dWs", dw_out="dWo", db_dil="db_dil", db_aux="db_dil",
               db_skip="db_skip", db_out="db_out")
ERR_UNSUPPORTED, ERR_NULL, ERR_WORKSPACE = -2, -4, -5  # pwg_status (include/pwg_kernels.h)

EDGE_TS = (1, 3, 4, 5, 31, 32, 33, 34, 35, 63, 64, 65, 96, 100, 131)
EDGE_DILS = (1, 2, 3, 4, 27, 32, 64, 512)
EDGE_GRID = [(T, dil) for T in EDGE_TS for dil in EDGE_DILS]
FINISH_NSL = (1, 2, 3, 4, 5, 9, 10, 11, 12, 13, 14, 15, 24, 25, 35, 36, 37, 47, 48, 49, 50)
FINISH_BIG = [(3, 5500, (3, 2)), (7, 7100, (7, 3))]  # (B, T, chunks per slice of the two launches)
SLICING = [(1, 32), (1, 20), (5, 32), (5, 7), (3, 96), (3, 95), (2, 160)]
SLICING_GRID = [(B, T, dil) for B, T in SLICING for dil in (1, 27)]
VARIANT_TS = (5, 100, 131)  # at dilation 3, B = 2


# ------------------------------------------------------------------------------------------------ inputs, references
@functools.lru_cache(maxsize=None)
def _data(B, T):
    """CPU float32 operands of the weight path at (B, T): its own inputs, no other kernel's result."""
    gen = torch.Generator().manual_seed(104729 * B + T)
    return {n: torch.randn(B, ROWS[n], T, generator=gen) for n in OPERANDS}


@functools.lru_cache(maxsize=None)
def _wn():
    """CPU float32 weight-norm tensors (v, g) of the four convolutions."""
    gen = torch.Generator().manual_seed(4242)
    return {n: (torch.randn(SHAPES[n], generator=gen), 0.5 + torch.rand(SHAPES[n][0], generator=gen)) for n in CONVS}


def _f64(B, T, with_go=True):
    t = _data(B, T)
    return [t[n].double() if n != "go" or with_go else None for n in OPERANDS]


@functools.lru_cache(maxsize=None)
def _ref(B, T, dil, with_go=True):
    return R.weight_backward(*_f64(B, T, with_go), dil)


@functools.lru_cache(maxsize=None)
def _ref_slabs(B, T, dil, per, with_go=True):
    return R.weight_backward_slabs(*_f64(B, T, with_go), dil, per)


def _place(t, device, off=0):
    """``t`` on the device, ``off`` floats past a 16-byte boundary."""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=device)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off
    return v


# ------------------------------------------------------------------------------------------------ one launch
def _launch(device, B, T, dil, with_go=True, db=BIASES, wn=(), dg=True, off=None, fill=None, tamper=None, expect=0):
    """One call of ``pwg_wavenet_weight_backward`` -> {name: CPU tensor} of the outputs asked for (``dw_*``, ``dg_*``,
    ``db_*``) plus the slabs read back from the workspace (``slab0``, ``slab1``) and the plan.

    ``db``: the convolutions whose bias gradient is asked for; ``wn``: the weight-normalised ones (``dg``: with dg);
    ``off`` = (operand, floats past a 16-byte boundary); ``fill``: what the workspace holds before the call;
    ``tamper(args)`` edits the call's arguments and ``expect`` is the status it must then return: a refusal, after
    which every buffer must still be the sentinel throughout."""
    t = _data(B, T)
    lib = _lib.lib()
    desc = ops.make_wavenet_desc(B, T, dil, out_mul=M.OUT_MUL, skip_mul=M.SKIP_MUL)
    plan = ops.wavenet_weight_backward_plan(desc)
    (s0, s1), per = plan["slices"], plan["chunks_per_slice"]
    nws = lib.pwg_wavenet_weight_backward_workspace_floats(ctypes.byref(desc))
    assert nws == s0 * 128 * (N0 + 1) + s1 * 128 * (N1 + 1)
    what = f"weight backward B{B} T{T} d{dil}"
    with poison_lds(), poison_empty():
        a = {n: _place(t[n], device, off[1] if off and off[0] == n else 0) for n in OPERANDS if n != "go" or with_go}
        a.setdefault("go", None)
        gd, keep = {}, []
        arr = (_lib.WaveNetParamGrad * 4)()
        for i, n in enumerate(CONVS):
            if n == "out" and not with_go:
                continue
            gd["dw_" + n] = M.Guarded(SHAPES[n], device)
            arr[i].dw = ops._ptr(gd["dw_" + n].out)
            if n in wn:
                keep += [x.to(device) for x in _wn()[n]]
                arr[i].v, arr[i].g = ops._ptr(keep[-2]), ops._ptr(keep[-1])
                if dg:
                    gd["dg_" + n] = M.Guarded(SHAPES[n][:1], device)
                    arr[i].dg = ops._ptr(gd["dg_" + n].out)
            if n in db:
                gd["db_" + n] = M.Guarded(SHAPES[n][:1], device)
                arr[i].db = ops._ptr(gd["db_" + n].out)
        ws = M.Guarded((nws,), device)
        if fill is not None:
            ws.out.fill_(fill)
        a.update(desc=desc, grads=arr, ws=ws.out, nws=nws)
        if tamper is not None:
            tamper(a)
        rc = lib.pwg_wavenet_weight_backward(None if a["desc"] is None else ctypes.byref(a["desc"]),
                                             *[ops._ptr(a[n]) for n in OPERANDS], a["grads"], ops._ptr(a["ws"]), a["nws"],
                                             ops._stream())
        if expect != 0:
            assert rc == expect, f"{what}: status {rc}, expected {expect}: {lib.pwg_last_error().decode(errors='replace')}"
            for n, g in list(gd.items()) + [("workspace", ws)]:
                assert bool((g.buf == M.SENTINEL).all()), f"{what}: {n} changed by a refused call"
            return lib.pwg_last_error().decode(errors="replace")
        assert rc == 0, f"{what}: status {rc}: {lib.pwg_last_error().decode(errors='replace')}"
        out = {n: g.check(f"{what}: {n}").cpu() for n, g in gd.items()}
        slabs = ws.check(f"{what}: workspace").cpu()
    for n, v in out.items():
        assert torch.isfinite(v).all(), f"{what}: {n} is not finite"
    out["slab0"] = slabs[:s0 * 128 * (N0 + 1)].view(s0, 128, N0 + 1)
    out["slab1"] = slabs[s0 * 128 * (N0 + 1):].view(s1, 128, N1 + 1)
    out["per"] = per
    return out


def _tensors(out):
    return {k: v for k, v in out.items() if k != "per"}


def _check_final(out, B, T, dil, with_go=True, what=""):
    """dw and db of the plain convolutions against float64 -> the worst error relative to the bar."""
    ref, worst = _ref(B, T, dil, with_go), 0.0
    for k, v in out.items():
        if k in REF_KEY and not (k.startswith("dw_") and "dg_" + k[3:] in out):
            err = M._err(v, ref[REF_KEY[k]])
            print(f"{what} {k}: rel-to-max error {err:.3e}")
            assert err <= RTOL, f"{what} {k}: rel-to-max error {err:.3e}"
            worst = max(worst, err)
    return worst


def _check_slabs(out, B, T, dil, with_go=True, what=""):
    """Every slab against float64, relative to the largest magnitude over all slabs of its launch."""
    refs, worst = _ref_slabs(B, T, dil, out["per"], with_go), 0.0
    for i, ref in enumerate(refs):
        got = out[f"slab{i}"].double()
        assert got.shape == ref.shape, (got.shape, ref.shape)
        assert torch.isfinite(got).all(), f"{what} slab{i}: not finite"
        diff = (got - ref).abs()
        err = diff.max().item() / (ref.abs().max().item() + 1e-12)
        s, m, col = [int(x) for x in torch.unravel_index(diff.argmax(), diff.shape)]
        print(f"{what} slab{i}: rel-to-max error {err:.3e}")
        assert err <= RTOL, (f"{what} slab{i}: rel-to-max error {err:.3e} at slice {s} (columns "
                             f"{R.slab_ranges(B, T, out['per'][i])[s]}), row {m}, column {col}: got {got[s, m, col].item()!r}, "
                             f"want {ref[s, m, col].item()!r}")
        worst = max(worst, err)
    return worst


def _same_bits(a, b, what):
    a, b = _tensors(a), _tensors(b)
    assert set(a) == set(b), (what, set(a) ^ set(b))
    M._same_bits(a, b, what)


# ------------------------------------------------------------------------------------------------ a. edge grid
@pytest.mark.parametrize("T,dil", EDGE_GRID, ids=[f"T{T}-d{dil}" for T, dil in EDGE_GRID])
def test_edge_grid(T, dil, device):
    """Final outputs and slabs against float64 at B = 2 with ``go`` and plain weights.  Measured: final outputs at most
    3.7e-7, slabs at most 4.5e-7 against the 2e-5 bar."""
    B = 2
    desc = ops.make_wavenet_desc(B, T, dil)
    chunks = B * -(-T // 32)
    per = 2 if chunks >= 2 else 1
    assert ops.wavenet_weight_backward_plan(desc) == dict(slices=(-(-chunks // per),) * 2, chunks_per_slice=(per,) * 2)
    out = _launch(device, B, T, dil)
    assert {k for k in out if k[:2] in ("dw", "db", "dg")} == {"dw_dil", "dw_aux", "dw_skip", "dw_out", "db_dil", "db_skip",
                                                               "db_out"}
    _check_slabs(out, B, T, dil, what="grid")
    _check_final(out, B, T, dil, what="grid")


# ------------------------------------------------------------------------------------------------ b. the finish, exactly
def _finish_ratio(out):
    """Worst |final - float64 sum of the float32 slabs| over the bound of counted roundings: an element is the sum of
    ``nsl`` slab terms in at most ``ceil(nsl / SL) + SL + 2`` additions (a lane's four accumulators over its share of the
    slices, their combination, the SL lane partials), each rounding at most 2^-24 of the sum of the absolute terms."""
    tot0 = torch.cat([out["dw_dil"].permute(0, 2, 1).reshape(128, 192), out["dw_aux"][:, :, 0], out["db_dil"][:, None]], 1)
    tot1 = torch.cat([torch.cat([out["dw_" + n][:, :, 0], out["db_" + n][:, None]], 1) for n in ("skip", "out")], 0)
    worst = 0.0
    for i, tot in enumerate((tot0, tot1)):
        slab = out[f"slab{i}"].double()
        nsl = slab.shape[0]
        bound = (-(-nsl // SL[i]) + SL[i] + 2) * U * slab.abs().sum(0)
        err = (tot.double() - slab.sum(0)).abs()
        assert bool((err[bound == 0] == 0).all()), f"launch {i}: a sum of zeros is not zero"
        worst = max(worst, (err / bound.clamp_min(1e-300)).max().item())
    return worst


@pytest.mark.parametrize("nsl", FINISH_NSL)
def test_finish_exact(nsl, device):
    """B = 1, T = 64 nsl - 17, dilation 3: both launches cut 2 nsl chunks into nsl slices of 2.  Measured: error / bound
    at most 0.32 (here and in ``test_finish_exact_long``)."""
    B, T, dil = 1, 64 * nsl - 17, 3
    assert ops.wavenet_weight_backward_plan(ops.make_wavenet_desc(B, T, dil)) == dict(slices=(nsl, nsl), chunks_per_slice=(2, 2))
    out = _launch(device, B, T, dil)
    ratio = _finish_ratio(out)
    print(f"nsl {nsl}: finish error / bound {ratio:.3f}")
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("B,T,per", FINISH_BIG, ids=[f"B{B}-T{T}" for B, T, _ in FINISH_BIG])
def test_finish_exact_long(B, T, per, device):
    """More than 512 and more than 1536 chunks: 3 and 2, then 7 and 3 chunks per slice, slices that straddle items with
    an odd number of chunks, 172 to 518 slices in the finish."""
    dil = 3
    plan = ops.wavenet_weight_backward_plan(ops.make_wavenet_desc(B, T, dil))
    assert plan["chunks_per_slice"] == per, plan
    chunks = B * -(-T // 32)
    assert plan["slices"] == tuple(-(-chunks // p) for p in per), plan
    out = _launch(device, B, T, dil)
    assert out["slab0"].shape[0] == plan["slices"][0] and out["slab1"].shape[0] == plan["slices"][1]
    ratio = _finish_ratio(out)
    print(f"B{B} T{T}: finish error / bound {ratio:.3f}")
    assert ratio <= 1.0, ratio


# ------------------------------------------------------------------------------------------------ c. slicing
@pytest.mark.parametrize("B,T,dil", SLICING_GRID, ids=[f"B{B}-T{T}-d{dil}" for B, T, dil in SLICING_GRID])
def test_slicing(B, T, dil, device):
    per_item = -(-T // 32)
    chunks = B * per_item
    per = 2 if chunks >= 2 else 1
    ranges = R.slab_ranges(B, T, per)
    assert ops.wavenet_weight_backward_plan(ops.make_wavenet_desc(B, T, dil)) == dict(slices=(len(ranges),) * 2,
                                                                                      chunks_per_slice=(per,) * 2)
    # what the case is there for
    if (B, T) in ((1, 32), (1, 20)):
        assert chunks == 1 and ranges == [[(0, 0, T)]]
    if (B, T) in ((5, 32), (5, 7)):
        assert per_item == 1 and len(ranges[0]) == 2 and len(ranges[-1]) == 1
    if (B, T) in ((3, 96), (3, 95)):
        assert any(len(r) == 2 for r in ranges) and chunks % 2 == 1  # a straddling slice; the last slice has one chunk
    out = _launch(device, B, T, dil)
    _check_slabs(out, B, T, dil, what="slicing")
    _check_final(out, B, T, dil, what="slicing")
    ratio = _finish_ratio(out)
    assert ratio <= 1.0, ratio


# ------------------------------------------------------------------------------------------------ d. variants
@pytest.mark.parametrize("T", VARIANT_TS)
def test_optional_outputs(T, device):
    B, dil = 2, 3
    base = _launch(device, B, T, dil)
    _check_slabs(base, B, T, dil, what="base")
    _check_final(base, B, T, dil, what="base")
    _same_bits(_launch(device, B, T, dil), base, "second launch")
    # the last layer: no go, grads[3] all NULL; rows 64 .. 127 of the second launch's slabs are zeros
    last = _launch(device, B, T, dil, with_go=False)
    assert not any(k.endswith("_out") for k in last)
    _check_slabs(last, B, T, dil, with_go=False, what="go=None")
    _check_final(last, B, T, dil, with_go=False, what="go=None")
    assert float(last["slab1"][:, 64:].abs().max()) == 0.0
    for k in last:
        if k not in ("slab1", "per"):
            assert torch.equal(last[k], base[k]), k
    assert torch.equal(last["slab1"][:, :64], base["slab1"][:, :64])
    # no bias gradient at all
    none = _launch(device, B, T, dil, db=())
    assert not any(k.startswith("db_") for k in none)
    _same_bits(none, {k: v for k, v in base.items() if not k.startswith("db_")}, "db=None")
    # a bias gradient for the aux convolution: the dilated convolution's, bit for bit
    aux = _launch(device, B, T, dil, db=CONVS)
    assert torch.equal(aux["db_aux"], aux["db_dil"])
    _same_bits({k: v for k, v in aux.items() if k != "db_aux"}, base, "grads[1].db given")
    # a dirty workspace
    for fill in (float("nan"), 3e38, -1e30):
        _same_bits(_launch(device, B, T, dil, fill=fill), base, f"workspace pre-filled with {fill}")


@pytest.mark.parametrize("T", VARIANT_TS)
def test_weight_norm(T, device):
    """(dv, dg) of each convolution alone and of all four, with and without dg, against ``R.weight_norm_backward`` of the
    float64 plain gradient; db and the gradients of the plain convolutions: the plain call's bits.  Measured: at most
    2.8e-7 against the 2e-5 bar."""
    B, dil = 2, 3
    base = _launch(device, B, T, dil)
    ref = _ref(B, T, dil)
    for wn in [(n,) for n in CONVS] + [CONVS]:
        with_dg = _launch(device, B, T, dil, wn=wn)
        for n in CONVS:
            if n not in wn:
                assert "dg_" + n not in with_dg and torch.equal(with_dg["dw_" + n], base["dw_" + n]), n
                continue
            v, g = _wn()[n]
            dv, dg = R.weight_norm_backward(ref[REF_KEY["dw_" + n]], v.double(), g.double())
            M._within(with_dg["dw_" + n], dv, f"wn={wn} dv_{n}", RTOL)
            M._within(with_dg["dg_" + n], dg, f"wn={wn} dg_{n}", RTOL)
        for k in [k for k in base if k[:2] == "db" or k[:4] == "slab"]:
            assert torch.equal(with_dg[k], base[k]), (wn, k)
        without = _launch(device, B, T, dil, wn=wn, dg=False)
        assert not any(k.startswith("dg_") for k in without)
        _same_bits(without, {k: v for k, v in with_dg.items() if not k.startswith("dg_")}, f"wn={wn}, dg=None")


@pytest.mark.parametrize("T", VARIANT_TS)
def test_operand_alignment(T, device):
    """The operand loads are declared 4-byte aligned (a row starts at ``row * T`` floats): each operand in turn 4, 8 and
    12 bytes past a 16-byte boundary gives the aligned call's bits."""
    B, dil = 2, 3
    base = _launch(device, B, T, dil)
    for name in OPERANDS:
        for off in (1, 2, 3):
            _same_bits(_launch(device, B, T, dil, off=(name, off)), base, f"{name} {4 * off} bytes off")


# ------------------------------------------------------------------------------------------------ e. refusals
def _set(key, value):
    return lambda a: a.__setitem__(key, value)


def _grad(i, **fields):
    def tamper(a):
        for k, v in fields.items():
            setattr(a["grads"][i], k, v)
    return tamper


def _other_desc(**kw):
    return _set("desc", ops.make_wavenet_desc(2, 35, 3, out_mul=M.OUT_MUL, skip_mul=M.SKIP_MUL, **kw))


REFUSALS = [(f"{n}=NULL", {}, _set(n, None), ERR_NULL, "NULL pointer") for n in ("dz", "x", "c", "gs", "g", "grads", "ws")]
REFUSALS += [(f"grads[{i}].dw=NULL", {}, _grad(i, dw=None), ERR_NULL, "NULL weight gradient") for i in range(3)]
REFUSALS += [
    ("desc=NULL", {}, _set("desc", None), ERR_UNSUPPORTED, "unsupported layer geometry"),
    ("go without grads[3].dw", {}, _grad(3, dw=None), ERR_NULL, "grads[3] goes with go"),
    ("grads[3].dw without go", {}, _set("go", None), ERR_NULL, "grads[3] goes with go"),
    ("v without g", dict(wn=("dil",)), _grad(0, g=None), ERR_NULL, "grads[0]: v, g (and dg) go together"),
    ("g without v", dict(wn=("skip",)), _grad(2, v=None, dg=None), ERR_NULL, "grads[2]: v, g (and dg) go together"),
    ("dg without v", dict(wn=("out",)), _grad(3, v=None, g=None), ERR_NULL, "grads[3]: v, g (and dg) go together"),
    ("workspace one short", {}, lambda a: a.__setitem__("nws", a["nws"] - 1), ERR_WORKSPACE, "workspace too small"),
    ("causal", {}, _other_desc(causal=True), ERR_UNSUPPORTED, "unsupported layer geometry"),
    ("aux_channels=72", {}, _other_desc(aux_channels=72), ERR_UNSUPPORTED, "unsupported layer geometry"),
    ("kernel=5", {}, _other_desc(kernel=5), ERR_UNSUPPORTED, "unsupported layer geometry"),
]


@pytest.mark.parametrize("kw,tamper,code,message", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_refusals(kw, tamper, code, message, device):
    """Every PWG_REQUIRE line of ``pwg_wavenet_weight_backward``: its status, its message, and every output and the
    workspace still the sentinel throughout."""
    said = _launch(device, 2, 35, 3, tamper=tamper, expect=code, **kw)
    assert message in said, said


# ------------------------------------------------------------------------------------------------ f. the layer
def test_layer_hands_the_kernel_the_operands_of_the_references(device):
    """``WaveNetResidualBlock`` (weight-normalised, fused) at T = 35, dilation 2 against float64 autograd: the parameter
    gradients -- from ``gs = skip_mul * ds_out`` and ``go`` as the autograd node forms them -- within LAYER_RTOL."""
    M.test_layer_autograd_matches_float64(2, 35, 2, True, M.SKIP_MUL, True, device)
