"""CPU: what the split-operand transposed convolution (csrc/conv1d_split.hip, ``convtr1d_split_mfma_kernel``; DESIGN.md
s9.3) covers and declines, its image size, and the admission predicate and module routing (pure host logic)."""
import torch

from parallelwavegan_amd import _lib, ops
from parallelwavegan_amd.layers import conv as conv_mod
from parallelwavegan_amd.layers.conv import Conv1d, ConvTranspose1d, upsample_split_admitted


def _desc(**kw):
    p = dict(batch=1, c_in=64, c_out=32, t_in=64, t_out=512, kernel=16, stride=8, pad_left=4, transposed=True)
    p.update(kw)
    return ops.make_conv_desc(p.pop("batch"), p.pop("c_in"), p.pop("c_out"), p.pop("t_in"), p.pop("t_out"),
                              p.pop("kernel"), **p)


def _reason():
    return _lib.lib().pwg_last_error().decode()


def test_supported_accepts_k_2s_with_tails_and_padded_rows():
    assert ops.convtr1d_split_supported(_desc())
    assert ops.convtr1d_split_supported(_desc(kernel=4, stride=2, pad_left=1, t_out=128))
    # channel tail (40 = 32 + 8), 72 rows padded to the 128-row tile; 48 rows padded to 64; 10 rows padded to 32
    assert ops.convtr1d_split_supported(_desc(c_in=40, c_out=9, pre_act="leaky_relu", pre_slope=0.1))
    assert ops.convtr1d_split_supported(_desc(c_in=40, c_out=24, kernel=4, stride=2, pad_left=1, t_out=128))
    assert ops.convtr1d_split_supported(_desc(c_in=33, c_out=5, kernel=4, stride=2, pad_left=1, t_out=128))
    # odd strides take the 4-byte epilogue (rows straddle channels): covered, not refused
    assert ops.convtr1d_split_supported(_desc(c_out=8, kernel=10, stride=5, pad_left=3, t_out=320))


def test_supported_refuses_what_is_out_of_scope_and_names_the_reason():
    assert not ops.convtr1d_split_supported(_desc(kernel=16, stride=4, pad_left=6, t_out=256))
    assert "convtr1d_split" in _reason() and "kernel == 2 * stride" in _reason()
    assert not ops.convtr1d_split_supported(_desc(groups=2))
    assert "groups" in _reason()
    assert not ops.convtr1d_split_supported(_desc(width=3))
    assert "width" in _reason()
    for mode in ("reflect", "replicate"):
        assert not ops.convtr1d_split_supported(_desc(pad_mode=mode))
        assert "zero padding" in _reason()
    stride1 = ops.make_conv_desc(1, 64, 64, 64, 64, 7, pad_left=3)
    assert ops.conv1d_split_supported(stride1) and not ops.convtr1d_split_supported(stride1)
    assert "convtr1d_split" in _reason() and "not a transposed convolution" in _reason()
    assert _lib.lib().pwg_convtr1d_split_packed_weight_bytes(stride1) == 0
    # and the stride-1 kernel keeps refusing the transposed descriptor, under its own name
    assert not ops.conv1d_split_supported(_desc())
    assert "conv1d_split: transposed" in _reason()


def test_image_is_three_bf16_transposed_images():
    lib = _lib.lib()
    for c_in, c_out, s in ((40, 9, 8), (64, 24, 2), (512, 256, 8)):
        d = _desc(c_in=c_in, c_out=c_out, kernel=2 * s, stride=s, pad_left=s // 2, t_out=64 * s)
        assert ops.conv1d_bf16_supported(d) and ops.convtr1d_split_supported(d)
        n = lib.pwg_convtr1d_split_packed_weight_bytes(d)
        assert n == 3 * lib.pwg_conv1d_bf16_packed_weight_bytes(d), (c_in, c_out, s)
        m = c_out * s
        m_pad = -(-m // 128) * 128 if m > 64 else (64 if m > 32 else 32)
        assert n == 3 * 2 * (-(-c_in // 32) * 32) * m_pad * 2, (c_in, c_out, s)  # 3 parts, 2 taps, bf16


def test_admission_predicate(monkeypatch):
    monkeypatch.setattr(conv_mod, "UPSAMPLE_SPLIT_ADMITTED", {(256, 128, 8): 6400})
    assert upsample_split_admitted(256, 128, 16, 8, 6400, False)
    assert not upsample_split_admitted(256, 128, 16, 8, 6399, False), "short launches stay on the fp32 kernel"
    assert not upsample_split_admitted(128, 64, 4, 2, 1 << 24, False), "a class that is not in the table"
    assert not upsample_split_admitted(256, 128, 8, 8, 1 << 24, False), "kernel != 2 * stride"
    assert not upsample_split_admitted(256, 128, 16, 8, 6400, True), "a gradient is needed"
    assert not upsample_split_admitted(256, 128, 16, 8, 6400, False, enabled=False), "the switch is off"
    assert upsample_split_admitted(64, 32, 4, 2, 1, False, admit_all=True)
    assert not upsample_split_admitted(64, 32, 4, 2, 1, True, admit_all=True)
    assert not upsample_split_admitted(64, 32, 4, 2, 1, False, enabled=False, admit_all=True)
    assert not upsample_split_admitted(64, 32, 6, 2, 1, False, admit_all=True)
    # never under the shortest launch that was measured, whatever the table says
    monkeypatch.setattr(conv_mod, "UPSAMPLE_SPLIT_ADMITTED", {(256, 128, 8): 1})
    assert not upsample_split_admitted(256, 128, 16, 8, conv_mod.UPSAMPLE_SPLIT_MIN_COLS - 1, False)
    assert upsample_split_admitted(256, 128, 16, 8, conv_mod.UPSAMPLE_SPLIT_MIN_COLS, False)


def test_module_routing_is_host_logic(monkeypatch):
    up = ConvTranspose1d(256, 128, 16, 8, padding=4)
    desc = up.make_desc(16, 6400)
    monkeypatch.setattr(conv_mod, "UPSAMPLE_SPLIT_ADMITTED", {(256, 128, 8): 1 << 16})
    monkeypatch.setattr(ConvTranspose1d, "split_exact", True)
    assert up._upsample_split_route(desc)
    assert not up._upsample_split_route(desc, needs_grad=True)
    assert not up._upsample_split_route(up.make_desc(1, 100)), "800 columns: under the class's column count"
    monkeypatch.setattr(ConvTranspose1d, "split_exact", False)
    assert not up._upsample_split_route(desc)
    monkeypatch.setattr(ConvTranspose1d, "split_exact", True)
    monkeypatch.setattr(ConvTranspose1d, "split_admit_all", True)
    assert up._upsample_split_route(up.make_desc(1, 100))
    assert not up._split_route(desc), "the stride-1 route keeps answering False for a transposed module"
    # what the kernel does not cover is not routed, admitted or not: k != 2s, groups; and never a stride-1 module
    k3s = ConvTranspose1d(256, 128, 24, 8, padding=8)
    assert not k3s._upsample_split_route(k3s.make_desc(16, 6400))
    grouped = ConvTranspose1d(256, 128, 16, 8, padding=4, groups=2)
    assert not grouped._upsample_split_route(grouped.make_desc(16, 6400))
    monkeypatch.setattr(Conv1d, "split_admit_all", True)
    cv = Conv1d(128, 128, 7, padding=3)
    assert not cv._upsample_split_route(cv.make_desc(16, 6400))


def test_admission_table_lists_only_measured_k_2s_classes():
    """Every key is a (c_in, c_out, stride) of HiFi-GAN V1's four upsampling layers -- the classes that were measured,
    all with kernel == 2 * stride -- and no class is admitted under the shortest launch measured on it: one utterance of
    100 frames, i.e. 100 x the upsampling factor up to and including the layer."""
    shortest = {(512, 256, 8): 800, (256, 128, 8): 6400, (128, 64, 2): 12800, (64, 32, 2): 25600}
    assert conv_mod.UPSAMPLE_SPLIT_MIN_COLS == min(shortest.values())
    for key, min_cols in conv_mod.UPSAMPLE_SPLIT_ADMITTED.items():
        assert key in shortest, key
        c_in, c_out, stride = key
        up = ConvTranspose1d(c_in, c_out, 2 * stride, stride, padding=stride // 2)
        assert up.kernel_size == 2 * up.stride and ops.convtr1d_split_supported(up.make_desc(1, 100))
        assert min_cols >= shortest[key], (key, min_cols)


def test_prepared_weights_hold_the_image_under_the_layer_key():
    """The image lives in the layer's PreparedWeights next to split(): one key, one staleness rule."""
    up = ConvTranspose1d(64, 32, 4, 2, padding=1)
    pw = up.prepared()
    assert pw._split_tr is None and pw._split is None
    assert up.prepared() is pw
    with torch.no_grad():
        up.weight.add_(1.0)
    assert up.prepared() is not pw, "a parameter update drops every image of the layer at once"
