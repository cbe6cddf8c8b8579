"""CPU: the arithmetic of the split-operand convolution (csrc/conv1d_split.hip) emulated in torch, what
the kernel's ``supported()`` declines, and the admission predicate of the routing (pure host logic)."""
import pytest
import torch

from parallelwavegan_amd import _lib, ops
from parallelwavegan_amd.layers import conv as conv_mod
from parallelwavegan_amd.layers.conv import Conv1d, ConvTranspose1d, split_admitted


def split3(v):
    """The packer's / the staging's split of an fp32 tensor: (hi, mid, lo) as fp32 tensors holding bf16 values."""
    hi = v.bfloat16().float()
    r = v - hi
    mid = r.bfloat16().float()
    lo = (r - mid).bfloat16().float()
    return hi, mid, lo


def _values():
    g = torch.Generator().manual_seed(7)
    v = torch.randn(1 << 16, generator=g) * torch.exp2(torch.randint(-20, 21, (1 << 16,), generator=g).float())
    edge = torch.tensor([0.0, -0.0, 1.0, -1.0, 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, 255.0 / 256, 3.0e38, 2.0 ** -100,
                         0.1, -0.1 * 0.1])
    return torch.cat([v, edge])


def test_three_way_split_is_exact():
    v = _values()
    hi, mid, lo = split3(v)
    # every step is exact in fp32: r and r - mid need no rounding, and the parts sum back to v in any order
    assert torch.equal((hi.double() + mid.double() + lo.double()).float(), v)
    assert torch.equal(hi.double() + mid.double() + lo.double(), v.double())
    assert torch.equal((v.double() - hi.double()).float().double(), v.double() - hi.double())
    # a 2-way split is not: hi + mid misses up to 2^-17 of |v|
    gap = (v.double() - hi.double() - mid.double()).abs()
    assert float(gap.max()) > 0
    assert bool((gap <= v.double().abs() * 2.0 ** -16).all())


def test_six_products_meet_the_bound():
    """On random data the six kept products, summed exactly, are within 3 * 2^-25 of sum |w x| of the exact dot product
    (the three dropped products mid.lo, lo.mid, lo.lo: 2^-24 each in the worst case, about 2^-28 on average)."""
    g = torch.Generator().manual_seed(11)
    w = torch.randn(64, 512, generator=g)
    x = torch.randn(512, 96, generator=g) * torch.exp2(torch.randint(-8, 9, (512, 1), generator=g).float())
    wp, xp = [p.double() for p in split3(w)], [p.double() for p in split3(x)]
    kept = [(2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)]  # (weight part, input part), the kernel's order
    six = sum(wp[a] @ xp[b] for a, b in kept)
    exact = w.double() @ x.double()
    bound = 3 * 2.0 ** -25 * (w.double().abs() @ x.double().abs())
    assert bool(((six - exact).abs() <= bound).all())
    # element-wise (worst case): |mid| <= 2^-8 |v| and |lo| <= 2^-16 |v|, so mid.lo <= 2^-24 and lo.lo <= 2^-32 of |w x|
    v = _values()
    hi, mid, lo = split3(v)
    assert bool((mid.double().abs() <= v.double().abs() * 2.0 ** -8).all())
    assert bool((lo.double().abs() <= v.double().abs() * 2.0 ** -16).all())


def _desc(**kw):
    p = dict(batch=1, c_in=32, c_out=32, t_in=64, t_out=64, kernel=7, stride=1, dilation=1, pad_left=3, groups=1)
    p.update(kw)
    return ops.make_conv_desc(p.pop("batch"), p.pop("c_in"), p.pop("c_out"), p.pop("t_in"), p.pop("t_out"),
                              p.pop("kernel"), **p)


def test_supported_declines_what_is_out_of_scope():
    assert ops.conv1d_split_supported(_desc())
    assert ops.conv1d_split_supported(_desc(kernel=11, dilation=5, pad_left=25, pre_act="leaky_relu", pre_slope=0.1))
    assert not ops.conv1d_split_supported(_desc(groups=2))
    assert not ops.conv1d_split_supported(_desc(width=3))
    assert not ops.conv1d_split_supported(_desc(pad_mode="reflect"))
    assert not ops.conv1d_split_supported(_desc(stride=2, t_out=32))
    assert not ops.conv1d_split_supported(_desc(kernel=16, stride=8, t_out=512, pad_left=4, transposed=True))
    assert b"conv1d_split" in _lib.lib().pwg_last_error()
    # three LDS planes: a window the bf16 kernel still takes can be too long for this one
    long_window = _desc(c_out=128, kernel=3, dilation=150, pad_left=150)
    assert ops.conv1d_bf16_supported(long_window) and not ops.conv1d_split_supported(long_window)
    assert _lib.lib().pwg_conv1d_split_packed_weight_bytes(_desc(groups=2)) == 0
    d = _desc(c_in=40, c_out=72)  # 2 chunks of 32 channels, 128 padded rows, 3 parts of bf16
    assert _lib.lib().pwg_conv1d_split_packed_weight_bytes(d) == 3 * 7 * 64 * 128 * 2
    # one image layout for both MFMA kernels: the split image is three bf16 images
    for c_out in (24, 64, 136, 512):
        for c_in in (24, 33, 80):
            d = _desc(c_in=c_in, c_out=c_out)
            assert ops.conv1d_bf16_supported(d) and ops.conv1d_split_supported(d)
            assert (_lib.lib().pwg_conv1d_split_packed_weight_bytes(d)
                    == 3 * _lib.lib().pwg_conv1d_bf16_packed_weight_bytes(d)), (c_in, c_out)


def test_admission_predicate(monkeypatch):
    monkeypatch.setattr(conv_mod, "SPLIT_ADMITTED", {(128, 128, 7): 1000})
    assert split_admitted(128, 128, 7, 1000, False)
    assert not split_admitted(128, 128, 7, 999, False), "short launches stay on the fp32 kernel"
    assert not split_admitted(128, 128, 3, 1 << 20, False), "a class that is not in the table"
    assert not split_admitted(128, 128, 7, 1000, True), "a gradient is needed"
    assert not split_admitted(128, 128, 7, 1000, False, enabled=False), "the switch is off"
    assert split_admitted(64, 64, 3, 1, False, admit_all=True)
    assert not split_admitted(64, 64, 3, 1, True, admit_all=True)
    assert not split_admitted(64, 64, 3, 1, False, enabled=False, admit_all=True)


def test_admission_table_names_only_wide_long_kernels():
    """What DESIGN.md s9.1 says of the table: k >= 7 at 128 / 256 channels, and no launch shorter than the shortest one
    measured to win (6400 columns; the 256-channel classes lose 2 - 3 x at 800)."""
    for (c_in, c_out, k), min_cols in conv_mod.SPLIT_ADMITTED.items():
        assert c_in == c_out and c_in in (128, 256) and k >= 7 and min_cols >= 6400, (c_in, c_out, k, min_cols)


def test_module_routing_is_host_logic(monkeypatch):
    cv = Conv1d(128, 128, 7, padding=3)
    desc = cv.make_desc(16, 51200)
    monkeypatch.setattr(conv_mod, "SPLIT_ADMITTED", {(128, 128, 7): 1 << 16})
    monkeypatch.setattr(Conv1d, "split_exact", True)
    assert cv._split_route(desc)
    assert not cv._split_route(desc, needs_grad=True)
    assert not cv._split_route(cv.make_desc(1, 800))
    monkeypatch.setattr(Conv1d, "split_exact", False)
    assert not cv._split_route(desc)
    monkeypatch.setattr(Conv1d, "split_exact", True)
    monkeypatch.setattr(Conv1d, "split_admit_all", True)
    assert cv._split_route(cv.make_desc(1, 800))
    assert not Conv1d(128, 128, 7, padding=3, groups=2)._split_route(Conv1d(128, 128, 7, padding=3, groups=2).make_desc(1, 800))
    monkeypatch.setattr(ConvTranspose1d, "split_admit_all", True)
    up = ConvTranspose1d(128, 64, 16, 8, padding=4)
    assert not up._split_route(up.make_desc(1, 800))


def test_abi_version_is_unchanged():
    assert _lib.lib().pwg_abi_version() == 15 and _lib.ABI_VERSION == 15
