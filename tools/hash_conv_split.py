"""SHA-256 of the output bytes of the MFMA convolutions (csrc/conv1d_split.hip, csrc/conv1d_bf16.hip and, for the bf16
weight image it reads, csrc/conv1d_stream_bf16.hip) and of the split-operand residual unit (csrc/resunit_split.hip) on a
fixed case list, as JSON on stdout: what a change of the kernels that must not change a bit is compared by (run this file
on both checkouts and compare the two objects).  GPU box only.  Every input is seeded on the CPU.
The split cases (the packed images are hashed next to the outputs): those of tests/test_conv_split_gpu.py (default
launch and 32x32x16); those of tests/test_conv_split_pipeline_gpu.py, whose shape / variant tables live here so that this
file also runs on a checkout that has no such test (default launch, tile_mode 1 / 2, 32x32x16, and the launches with one
operand 4 bytes off a 16-byte boundary); and the four admitted classes (128 / 256 channels, k = 7 / 11) at one utterance
of 100 frames with dilations 1 and 5, at tile_mode 0 / 1 / 2 and both MFMA shapes.
The bf16 cases: every case of tests/test_conv_bf16_gpu.py::ALL, the packed image and the output at both MFMA shapes;
and pushes through the bf16 stream kernel on layers whose rows are padded in the image (y and hist_out).
The unit cases: the CASES of tests/test_resunit_split_gpu.py with that file's inputs, the table kept here as for the
pipeline cases; ``ops.resunit_forward_split`` at both MFMA shapes."""
import hashlib
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

# name -> B, cin, cout, T, k, dil, pad_left (t_out = T: zeros on the right make up the rest of the receptive field)
PIPELINE_SHAPES = {
    # a single chunk; second row block with padded rows; first, interior and partial column tiles; window shift 3
    "one_chunk": dict(B=1, cin=24, cout=136, T=300, k=3, dil=1, pad_left=1),
    # whole chunks, 16-byte staging, shift 1, interior tiles
    "two_chunks": dict(B=2, cin=64, cout=128, T=516, k=7, dil=1, pad_left=3),
    # odd chunk count, 8-channel chunk tail, the widest window, padded rows
    "three_chunks_tail": dict(B=2, cin=72, cout=72, T=640, k=11, dil=5, pad_left=25),
    # no next tap; shift 0
    "one_tap": dict(B=1, cin=96, cout=128, T=260, k=1, dil=1, pad_left=0),
    # halo on the left only; 64-row tile
    "causal": dict(B=1, cin=64, cout=64, T=512, k=3, dil=2, pad_left=4),
    # 32-row tile; T % 4 != 0: 4-byte staging and the epilogue's 4-byte path; shift 2
    "narrow": dict(B=2, cin=40, cout=24, T=515, k=5, dil=1, pad_left=2),
    # T under one tile, one-channel chunk tail, row tail, per-item base pointers
    "tiny": dict(B=3, cin=33, cout=33, T=37, k=3, dil=1, pad_left=1),
}

# every epilogue / activation switch alone, and all together
PIPELINE_VARIANTS = {
    "plain": dict(),
    "bias": dict(bias=True),
    "add1": dict(add1=True),
    "add2": dict(add2=True),
    "mul": dict(out_mul=0.5),
    "div3": dict(out_div=3.0),
    "post_lrelu": dict(post_act="leaky_relu", post_slope=0.1),
    "post_relu": dict(post_act="relu"),
    "post_tanh": dict(post_act="tanh"),
    "pre_lrelu": dict(pre_act="leaky_relu", pre_slope=0.1),
    "pre_relu": dict(pre_act="relu"),
    "all": dict(bias=True, add1=True, add2=True, out_mul=0.5, out_div=3.0, pre_act="leaky_relu", pre_slope=0.1,
                post_act="tanh"),
}
ALL_VARIANT_SHAPES = ("one_chunk", "three_chunks_tail")
ALIGN_SHAPES = ("two_chunks", "three_chunks_tail", "one_tap")
# (shape, variant, input kind); kinds as in tests/test_conv_split_gpu.py
PIPELINE_CASES = ([(s, v, "randn") for s in ALL_VARIANT_SHAPES for v in PIPELINE_VARIANTS]
                  + [(s, v, "randn") for s in PIPELINE_SHAPES if s not in ALL_VARIANT_SHAPES for v in ("plain", "all")]
                  + [("three_chunks_tail", "plain", "wide"), ("three_chunks_tail", "plain", "cancel")])


def pipeline_variant(name):
    v = dict(bias=False, add1=False, add2=False, out_mul=1.0, out_div=1.0, pre_act=None, pre_slope=0.0, post_act=None,
             post_slope=0.0)
    v.update(PIPELINE_VARIANTS[name])
    return v


def pipeline_inputs(shape, kind):
    """CPU float32 operands of a pipeline case (the kinds of tests/test_conv_split_gpu.py::_inputs)."""
    s = PIPELINE_SHAPES[shape]
    g = torch.Generator().manual_seed(sum(map(ord, shape + kind)) * 977 + s["T"])
    x = torch.randn(s["B"], s["cin"], s["T"], generator=g)
    w = torch.randn(s["cout"], s["cin"], s["k"], generator=g) / (s["cin"] * s["k"]) ** 0.5
    if kind == "wide":
        e = torch.linspace(-20, 20, s["cin"])[torch.randperm(s["cin"], generator=g)]
        x = x * torch.exp2(e.round()).view(1, -1, 1)
    if kind == "cancel":
        u = torch.rand(s["B"], s["cin"] // 2, s["T"], generator=g) * 2 - 1
        x[:, 1::2] = x[:, 0::2] * (1 + u / 16)
        w[:, 1::2] = -w[:, 0::2]
    bias = torch.randn(s["cout"], generator=g)
    add1 = torch.randn(s["B"], s["cout"], s["T"], generator=g)
    add2 = torch.randn(s["B"], s["cout"], s["T"], generator=g)
    return dict(x=x, w=w, bias=bias, add1=add1, add2=add2)


def pipeline_desc(shape, variant):
    from parallelwavegan_amd import ops

    s, v = PIPELINE_SHAPES[shape], pipeline_variant(variant)
    return ops.make_conv_desc(s["B"], s["cin"], s["cout"], s["T"], s["T"], s["k"], 1, s["dil"], s["pad_left"],
                              pre_act=v["pre_act"], pre_slope=v["pre_slope"], post_act=v["post_act"],
                              post_slope=v["post_slope"], out_mul=v["out_mul"], out_div=v["out_div"])


def off_by_4_bytes(t):
    """A copy of t that starts 4 bytes after a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def hash_existing(out, dev):
    from parallelwavegan_amd import ops
    from tests import test_conv_split_gpu as ex

    for shape, variant, kind in ex.CASES:
        s, v, t = ex.SHAPES[shape], ex._variant(variant), ex._inputs(shape, kind)
        pad = (s["k"] - 1) // 2 * s["dil"]
        desc = ops.make_conv_desc(s["B"], s["cin"], s["cout"], s["T"], s["T"], s["k"], 1, s["dil"], pad,
                                  pre_act=v["pre_act"], pre_slope=v["pre_slope"], post_act=v["post_act"],
                                  out_div=v["out_div"])
        x, ws = t["x"].to(dev), ops.pack_weight_split(desc, t["w"].to(dev))
        out[f"split_gpu/{shape}-{variant}-{kind}/image"] = sha(ws)
        bias, add1, add2 = (t[n].to(dev) if v[n] else None for n in ("bias", "add1", "add2"))
        for shp in (16, 32):
            y = ops.conv1d_forward_split(desc, x, ws, bias, add1, add2, mfma_shape=shp)
            out[f"split_gpu/{shape}-{variant}-{kind}/mfma{shp}"] = sha(y)


def hash_pipeline(out, dev):
    from parallelwavegan_amd import ops

    for shape, variant, kind in PIPELINE_CASES:
        v, t = pipeline_variant(variant), pipeline_inputs(shape, kind)
        desc = pipeline_desc(shape, variant)
        x, ws = t["x"].to(dev), ops.pack_weight_split(desc, t["w"].to(dev))
        bias, add1, add2 = (t[n].to(dev) if v[n] else None for n in ("bias", "add1", "add2"))
        name = f"pipeline/{shape}-{variant}-{kind}"
        out[f"{name}/image"] = sha(ws)
        for mode in (0, 1, 2):
            out[f"{name}/tile{mode}"] = sha(ops.conv1d_forward_split(desc, x, ws, bias, add1, add2, tile_mode=mode))
        out[f"{name}/mfma32"] = sha(ops.conv1d_forward_split(desc, x, ws, bias, add1, add2, mfma_shape=32))
    for shape in ALIGN_SHAPES:
        t = pipeline_inputs(shape, "randn")
        desc = pipeline_desc(shape, "all")
        ws = ops.pack_weight_split(desc, t["w"].to(dev))
        for which in ("x", "add1", "add2", "out"):
            arg = {n: t[n].to(dev) for n in ("x", "bias", "add1", "add2")}
            y = None
            if which == "out":
                y = off_by_4_bytes(torch.zeros(t["add1"].shape, device=dev))
            else:
                arg[which] = off_by_4_bytes(arg[which])
            y = ops.conv1d_forward_split(desc, arg["x"], ws, arg["bias"], arg["add1"], arg["add2"], out=y)
            out[f"pipeline/{shape}-all-randn/{which}_off4"] = sha(y)


def hash_admitted(out, dev):
    from parallelwavegan_amd import ops

    for ch, T in ((256, 800), (128, 6400)):  # HiFi-GAN V1 stages 1 and 2 at one utterance of 100 frames
        for k in (7, 11):
            for d in (1, 5):
                g = torch.Generator().manual_seed(ch * 1000 + k * 10 + d)
                w = torch.randn(ch, ch, k, generator=g) * 0.05
                x, bias = torch.randn(1, ch, T, generator=g), torch.randn(ch, generator=g)
                add1 = torch.randn(1, ch, T, generator=g)
                desc = ops.make_conv_desc(1, ch, ch, T, T, k, dilation=d, pad_left=(k - 1) // 2 * d,
                                          pre_act="leaky_relu", pre_slope=0.1)
                ws = ops.pack_weight_split(desc, w.to(dev))
                out[f"admitted/c{ch}_k{k}_d{d}_T{T}/image"] = sha(ws)
                x, bias, add1 = x.to(dev), bias.to(dev), add1.to(dev)
                for mode in (0, 1, 2):
                    for shp in (16, 32):
                        y = ops.conv1d_forward_split(desc, x, ws, bias, add1, tile_mode=mode, mfma_shape=shp)
                        out[f"admitted/c{ch}_k{k}_d{d}_T{T}/tile{mode}/mfma{shp}"] = sha(y)


def hash_bf16(out, dev):
    from parallelwavegan_amd import ops
    from tests import test_conv_bf16_gpu as ex

    for c in ex.ALL:
        g = torch.Generator().manual_seed(c["B"] * 7919 + c["Cin"] * 31 + c["K"] * 7 + c["T"])
        B, cin, cout, T, K, s, d = c["B"], c["Cin"], c["Cout"], c["T"], c["K"], c["stride"], c["dil"]
        x = torch.randn(B, cin, T, generator=g)
        if c["transposed"]:
            w = torch.randn(cin, cout, K, generator=g) / (cin * 2) ** 0.5
            pad = s // 2 + s % 2
            t_out = ops.conv_transpose_out_length(T, K, s, pad, s % 2)
        else:
            w = torch.randn(cout, cin, K, generator=g) / (cin * K) ** 0.5
            pad, t_out = (K - 1) // 2 * d, T
        bias, add1, add2 = torch.randn(cout, generator=g), torch.randn(B, cout, t_out, generator=g), \
            torch.randn(B, cout, t_out, generator=g)
        bias, add1, add2 = (t.to(dev) if c[n] else None for n, t in (("bias", bias), ("add1", add1), ("add2", add2)))
        desc = ops.make_conv_desc(B, cin, cout, T, t_out, K, stride=s, dilation=d, pad_left=pad,
                                  transposed=c["transposed"], pre_act=c["pre"], pre_slope=c["slope"] if c["pre"] else 0.0,
                                  post_act=c["post"], post_slope=c["post_slope"], out_mul=c["mul"], out_div=c["div"])
        wp = ops.pack_weight_bf16(desc, w.to(dev))
        out[f"bf16/{ex._id(c)}/image"] = sha(wp)
        for shp in (16, 32):
            y = ops.conv1d_forward_bf16(desc, x.to(dev), wp, bias, add1, add2, mfma_shape=shp)
            out[f"bf16/{ex._id(c)}/mfma{shp}"] = sha(y)


# name -> c_in, c_out, k, dilation, transposed stride (0: Conv1d), start-of-stream padding, columns per push: the rows
# of every image are padded (c_out 33 / 40; 33 * 4 phases), c_in 20 is a partial chunk, 160 a block and a chunk
STREAM_CASES = {
    "c20_o40_k7_zero": (20, 40, 7, 1, 0, "zero", (5, 17, 33)),
    "c160_o33_k5_d3_zero": (160, 33, 5, 3, 0, "zero", (17, 5, 33)),
    "c160_o40_k7_replicate": (160, 40, 7, 1, 0, "replicate", (33, 5, 17)),
    "t_c20_o33_k8_s4_replicate": (20, 33, 8, 1, 4, "replicate", (5, 17, 33)),
}


def hash_stream_bf16(out, dev):
    from parallelwavegan_amd import ops

    for name, (cin, cout, k, d, s, mode, pushes) in STREAM_CASES.items():
        g = torch.Generator().manual_seed(sum(map(ord, name)) * 131 + cin)
        B, H = 2, 1 if s else (k - 1) * d
        w = torch.randn((cin, cout, k) if s else (cout, cin, k), generator=g) / (cin * k) ** 0.5
        bias = torch.randn(cout, generator=g).to(dev)
        wp, hist = None, None
        for i, n in enumerate(pushes):
            x = torch.randn(B, cin, n, generator=g).to(dev)
            if s:
                desc = ops.make_conv_desc(B, cin, cout, n, n * s, k, s, 1, s, transposed=True, pad_mode=mode,
                                          pre_act="leaky_relu", pre_slope=0.1)
            else:
                desc = ops.make_conv_desc(B, cin, cout, n, n, k, 1, d, H, pad_mode=mode, pre_act="leaky_relu",
                                          pre_slope=0.1)
            if wp is None:
                wp = ops.pack_weight_bf16(desc, w.to(dev))
                out[f"stream_bf16/{name}/image"] = sha(wp)
            hist_out = torch.full((B, cin, H), float("nan"), device=dev)
            y = ops.conv1d_stream_forward_bf16(desc, x, hist, hist_out, wp, bias)
            out[f"stream_bf16/{name}/push{i}_n{n}/y"] = sha(y)
            out[f"stream_bf16/{name}/push{i}_n{n}/hist_out"] = sha(hist_out)
            hist = hist_out


# (C, k, d, pair, batch, T, variant, kind): the CASES of tests/test_resunit_split_gpu.py
UNIT_KD = [(3, 1), (3, 5), (7, 3), (11, 1), (11, 5)]
UNIT_BT = [(2, 100), (3, 1000), (2, 4148)]
UNIT_VARIANTS = {
    "plain": dict(bias=False, add2=False, out_div=1.0),
    "all": dict(bias=True, add2=True, out_div=3.0),
    "bias": dict(bias=True, add2=False, out_div=1.0),
    "add2": dict(bias=False, add2=True, out_div=1.0),
    "div3": dict(bias=False, add2=False, out_div=3.0),
}
UNIT_CASES = ([(c, k, d, pair, b, t, v, "randn") for c, (k, d), pair, (b, t), v
               in itertools.product((32, 64), UNIT_KD, (True, False), UNIT_BT, ("plain", "all"))]
              + [(32, 7, 3, True, 3, 1000, v, "randn") for v in ("bias", "add2", "div3")]
              + [(64, 3, 5, False, 3, 1000, v, "randn") for v in ("bias", "add2", "div3")]
              + [(64, 7, 3, True, 3, 1000, "all", "wide"), (32, 11, 5, True, 3, 1000, "plain", "wide"),
                 (64, 11, 5, True, 3, 1000, "plain", "cancel"), (32, 7, 3, True, 3, 1000, "all", "cancel")])


def unit_inputs(c, k, b, t, kind):
    """CPU float32 operands of a unit case (tests/test_resunit_split_gpu.py::_inputs)."""
    g = torch.Generator().manual_seed(c * 100003 + k * 1009 + b * 101 + t + len(kind))
    x = torch.randn(b, c, t, generator=g)
    w1 = torch.randn(c, c, k, generator=g) / (c * k) ** 0.5
    w2 = torch.randn(c, c, k, generator=g) / (c * k) ** 0.5
    if kind == "wide":
        e = torch.linspace(-20, 20, c)[torch.randperm(c, generator=g)]
        x = x * torch.exp2(e.round()).view(1, -1, 1)
    if kind == "cancel":
        u = torch.rand(b, c // 2, t, generator=g) * 2 - 1
        x[:, 1::2] = x[:, 0::2] * (1 + u / 16)
        w1[:, 1::2] = -w1[:, 0::2]
    return dict(x=x, w1=w1, w2=w2, b1=torch.randn(c, generator=g), b2=torch.randn(c, generator=g),
                add2=torch.randn(b, c, t, generator=g))


def hash_unit(out, dev):
    from parallelwavegan_amd import ops

    for c, k, d, pair, b, t, variant, kind in UNIT_CASES:
        i, v = unit_inputs(c, k, b, t, kind), UNIT_VARIANTS[variant]
        desc = ops.make_resunit_desc(b, c, t, k, d, pair, 0.1, 0.1, v["out_div"])
        wdesc = ops.make_conv_desc(1, c, c, 64, 64, k, pad_left=(k - 1) // 2)
        i1 = ops.pack_weight_split(wdesc, i["w1"].to(dev))
        i2 = ops.pack_weight_split(wdesc, i["w2"].to(dev)) if pair else None
        b1 = i["b1"].to(dev) if v["bias"] else None
        b2 = i["b2"].to(dev) if v["bias"] and pair else None
        add2 = i["add2"].to(dev) if v["add2"] else None
        name = "unit/c%d_k%d_d%d_%s_b%d_t%d-%s-%s" % (c, k, d, "pair" if pair else "single", b, t, variant, kind)
        for shp in (16, 32):
            y = ops.resunit_forward_split(desc, i["x"].to(dev), i1, b1, i2, b2, add2, mfma_shape=shp)
            out[f"{name}/mfma{shp}"] = sha(y)


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    hashes = {}
    hash_existing(hashes, dev)
    hash_pipeline(hashes, dev)
    hash_admitted(hashes, dev)
    hash_bf16(hashes, dev)
    hash_stream_bf16(hashes, dev)
    hash_unit(hashes, dev)
    print(json.dumps({"hashes": len(hashes), "sha256": hashes}, indent=1, sort_keys=True))
