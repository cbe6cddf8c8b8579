"""Do two builds of the library dispatch the conv forward and data gradient alike?  (PWG_KERNEL_LIB names the other one.)

--digest (host only, no GPU): one sha256 over the dispatcher's answers.  Hashed in a fixed order, per descriptor: the
status code and, where it is 0, the eight integers of ``pwg_conv1d_plan`` with has_addends 0 and 1 (out[] is not written
on a refusal), then ``pwg_conv1d_forward_workspace_floats`` and ``pwg_conv1d_backward_data_workspace_floats``.
Descriptors, each under the concurrency hints 1.0 and 0.25:
  * the named ones: every shape of tests/test_conv_cfg_matrix_gpu.py, the planner cases of tests/test_tile_order.py, the
    rows of tests/test_conv_plan_host.py and one descriptor per refusal of make_geometry;
  * the sweep: channels x channels x k x stride x dilation x groups x width x batch x t_out x (plain, transposed) x pad
    mode, 128.3 million points, of which every STEP-th is taken (STEP is prime and divides no axis length, so the walk
    visits every value of every axis and mixes them).  Points whose groups do not divide the channels are dropped.
    "Same" padding (plain: (k - 1) * dilation / 2 on both sides; transposed: (k - stride) / 2), so the refusals come by
    themselves: a reflect pad of t_in or more, reflect at width > 1, transposed under a pad mode or with dilation and
    stride above 1.
The digest is about the dispatcher without overrides and refuses to run when a PWG_* variable other than PWG_KERNEL_LIB is
set, unless ``--allow-override NAME`` names it; ``--overrides`` runs itself once per override of OVERRIDE_RUNS in a
subprocess and prints each digest.

--hash (GPU, one process, a few seconds): sha256 of the output bytes of ``ops.conv1d_forward`` and
``ops.conv1d_backward_data`` on every shape x variant / mode of tests/test_conv_cfg_matrix_gpu.py, one call each of the
single-input-channel and the two few-output-channel routes in both directions, and ``ops.conv1d_forward_cfg`` on S1 and S5
for all 20 tiles on both staging paths -- the launch fields the plan does not expose (x-row stride, LDS bytes, FAST and
pre-activation variant, epilogue mode) all change bits or fault when they are wrong.

Usage: python tools/sweep_conv_plan.py --digest [--step 101] [--allow-override NAME ...] | --overrides | --hash
"""
import argparse
import ctypes
import hashlib
import os
import struct
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from parallelwavegan_amd import _lib, ops  # noqa: E402

CHANNELS = (1, 3, 4, 20, 32, 48, 64, 96, 128, 256, 512, 1024)
AXES = (  # slowest first
    ("c_in", CHANNELS), ("c_out", CHANNELS), ("k", (1, 3, 4, 5, 7, 8, 11, 15, 16, 41, 63)), ("stride", (1, 2, 3, 4, 8)),
    ("dil", (1, 3, 9, 27, 243)), ("groups", (1, 4, 16)), ("width", (1, 2, 3, 5, 11)), ("batch", (1, 2, 16, 64)),
    ("t_out", (7, 9, 32, 100, 260, 2048, 8192, 51200, 204800)), ("transposed", (False, True)),
    ("pad_mode", ("zero", "reflect", "replicate")),
)
HINTS = (1.0, 0.25)
OVERRIDE_RUNS = (("PWG_TILE_ORDER", "2"), ("PWG_ROWS32", "0"), ("PWG_SPLIT_FILL", "0"), ("PWG_SPLIT_UNDERFILL", "0"),
                 ("PWG_FORCE_CFG", "2,4"))


def sweep_desc(p):
    if p["c_in"] % p["groups"] or p["c_out"] % p["groups"]:
        return None
    k, s, dil, t_out = p["k"], p["stride"], p["dil"], p["t_out"]
    if p["transposed"]:
        pad, t_in = max(k - s, 0) // 2, -(-t_out // s)
    else:
        pad, t_in = (k - 1) * dil // 2, (t_out - 1) * s + 1 + (k - 1) * dil - 2 * ((k - 1) * dil // 2)
    return ops.make_conv_desc(p["batch"], p["c_in"], p["c_out"], t_in, t_out, k, s, dil, pad, p["groups"],
                              transposed=p["transposed"], width=p["width"], pad_mode=p["pad_mode"])


def sweep(step):
    total = 1
    for _, values in AXES:
        total *= len(values)
    assert all(step % len(values) for _, values in AXES if len(values) > 1) and step > 1
    for i in range(0, total, step):
        p = {}
        for name, values in reversed(AXES):
            i, r = divmod(i, len(values))
            p[name] = values[r]
        d = sweep_desc(p)
        if d is not None:
            yield d


def named():
    from tests import test_conv_cfg_matrix_gpu as m
    from tests import test_conv_plan_host as h

    for s in m.SHAPES:
        yield m._desc(s, m._variant("plain"))

    def same(batch, c_in, c_out, t_in, k, stride=1, width=1, t_out=None, groups=1):
        pad = (k - 1) // 2
        if t_out is None:
            t_out = ops.conv_out_length(t_in, k, stride, 1, pad, pad)
        return ops.make_conv_desc(batch, c_in, c_out, t_in, t_out, k, stride, 1, pad, groups, width=width)

    # tests/test_tile_order.py: _PLANNER_CASES, the other kernel families, the grid product
    for t in (9, 17, 32):
        yield same(16, 1024, 1024, t, 5)
    yield same(16, 1024, 1024, 21, 5, width=5)
    yield same(16, 512, 1024, 61, 5, stride=3, width=5, t_out=21)
    for c, t, k in ((128, 51200, 11), (256, 6400, 7), (64, 102400, 3), (512, 800, 7)):
        yield same(16, c, c, t, k)
    yield same(1, 1024, 1024, 32, 5)
    yield same(16, 1, 128, 8192, 15)
    yield same(16, 32, 1, 204800, 7)
    for b in (1, 16):
        for c_in in (64, 1024):
            for c_out in (128, 1024):
                for t in (9, 300):
                    for k in (3, 5):
                        for s in (1, 3):
                            yield ops.make_conv_desc(b, c_in, c_out, t, ops.conv_out_length(t, k, s, 1, k // 2, k // 2), k, s,
                                                     1, k // 2, 1)
    for row in h.ROWS:
        yield h.make_desc(row)
    # make_geometry's refusals: negative padding, a size of 0, groups that do not divide, an output that starts past the
    # input, a reflect pad of t_in, reflect / replicate at width 2, transposed under a pad mode / with dilation and stride
    yield ops.make_conv_desc(2, 32, 32, 100, 100, 3, 1, 1, -1, 1)
    yield ops.make_conv_desc(2, 32, 32, 0, 100, 3, 1, 1, 1, 1)
    yield ops.make_conv_desc(2, 32, 48, 100, 100, 3, 1, 1, 1, 5)
    yield ops.make_conv_desc(2, 32, 32, 10, 100, 3, 1, 1, 1, 1)
    yield ops.make_conv_desc(2, 32, 32, 28, 28, 3, 1, 28, 28, 1, pad_mode="reflect")
    yield ops.make_conv_desc(2, 32, 32, 28, 28, 3, 1, 1, 1, 1, width=2, pad_mode="reflect")
    yield ops.make_conv_desc(2, 32, 32, 28, 28, 3, 1, 1, 1, 1, width=2, pad_mode="replicate")
    yield ops.make_conv_desc(2, 32, 32, 28, 56, 4, 2, 1, 1, 1, transposed=True, pad_mode="replicate")
    yield ops.make_conv_desc(2, 32, 32, 28, 56, 4, 2, 3, 1, 1, transposed=True)


def digest(args):
    lib = _lib.lib()
    plan, ws_f, ws_b = lib.pwg_conv1d_plan, lib.pwg_conv1d_forward_workspace_floats, lib.pwg_conv1d_backward_data_workspace_floats
    out = (ctypes.c_int32 * 8)()
    h = hashlib.sha256()
    queries = refused = descs = 0
    was = lib.pwg_set_concurrency_hint(1.0)
    for hint in HINTS:
        lib.pwg_set_concurrency_hint(hint)
        for source in (named(), sweep(args.step)):
            for d in source:
                ref = ctypes.byref(d)
                descs += 1
                for addends in (0, 1):
                    rc = plan(ref, addends, out)
                    refused += rc != 0
                    h.update(struct.pack("<i", rc))
                    if rc == 0:
                        h.update(bytes(out))
                h.update(struct.pack("<QQ", ws_f(ref), ws_b(ref)))
                queries += 4
    lib.pwg_set_concurrency_hint(was)
    allowed = " ".join(f"{k}={os.environ[k]}" for k in sorted(args.allow_override) if k in os.environ)
    print(f"{_lib.LIB_PATH}: {descs} descriptors, {queries} queries, {refused} plans refused, --step {args.step}"
          + (f", under {allowed}" if allowed else ""))
    print("sha256 " + h.hexdigest())


def overrides(args):
    for name, value in OVERRIDE_RUNS:
        env = dict(os.environ, **{name: value})
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--digest", "--step", str(args.step),
                            "--allow-override", name], env=env, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(r.stdout + r.stderr)
        print(r.stdout, end="")


def output_hashes():
    import torch

    from tests import test_conv_cfg_matrix_gpu as m

    dev = torch.device("cuda:0")

    def show(what, t):
        torch.cuda.synchronize()
        print(f"{hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()}  {what}")

    for shape in m.SHAPES:
        for variant in m.VARIANTS:
            v = m._variant(variant)
            desc = m._desc(shape, v)
            x, w, bias, add1, add2 = m._dev(shape, dev, "x", "w", "bias", "add1", "add2")
            wp = ops.pack_weight(desc, w)
            show(f"forward {shape} {variant}", ops.conv1d_forward(desc, x, wp, bias if v["bias"] else None,
                                                                   add1 if v["add1"] else None, add2 if v["add2"] else None))
    for shape in m.BWD_SHAPES:
        for mode, (pre_act, pre_slope, with_accum) in m.BWD_MODES.items():
            v = m._variant("plain")
            v.update(pre_act=pre_act, pre_slope=pre_slope)
            desc = m._desc(shape, v)
            dy, w, xz, accum = m._dev(shape, dev, "dy", "w", "xz", "accum")
            wb = ops.pack_weight_bwd(desc, w)
            show(f"backward_data {shape} {mode}", ops.conv1d_backward_data(desc, dy, wb, xz if pre_act else None,
                                                                            accum if with_accum else None))
    # the streaming routes, forward and (for the layer whose data gradient is such a convolution) backward
    g = torch.Generator().manual_seed(7)
    for what, (b, cin, cout, k, t) in (("single input channel", (2, 1, 16, 15, 2048)), ("few outputs, LDS", (1, 8, 2, 9, 4096)),
                                       ("few outputs, stream", (1, 8, 1, 7, 4096))):
        for c_in, c_out in ((cin, cout), (cout, cin)):
            desc = ops.make_conv_desc(b, c_in, c_out, t, t, k, 1, 1, (k - 1) // 2, 1)
            x = torch.randn(b, c_in, t, generator=g).to(dev)
            w = (torch.randn(c_out, c_in, k, generator=g) / (c_in * k) ** 0.5).to(dev)
            dy = torch.randn(b, c_out, t, generator=g).to(dev)
            plan = ops.conv1d_plan(desc)["family"]
            show(f"forward {what} {c_in}->{c_out} ({plan})", ops.conv1d_forward(desc, x, ops.pack_weight(desc, w), None))
            show(f"backward_data {what} {c_in}->{c_out}", ops.conv1d_backward_data(desc, dy, ops.pack_weight_bwd(desc, w)))
    for shape in ("S1", "S5"):
        v = m._variant("mrf")
        desc = m._desc(shape, v)
        x, w, bias, add1, add2 = m._dev(shape, dev, "x", "w", "bias", "add1", "add2")
        wp = ops.pack_weight(desc, w)
        for cfg in range(ops.num_tile_configs()):
            for dma in (True, False):
                show(f"forward_cfg {shape} mrf cfg {cfg} dma={dma}",
                     ops.conv1d_forward_cfg(desc, x, wp, bias, add1, add2, tile_config=cfg, use_dma=dma))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--digest", action="store_true", help="one hash of every plan and workspace answer (host only)")
    ap.add_argument("--overrides", action="store_true", help="--digest under each override of OVERRIDE_RUNS, one subprocess each")
    ap.add_argument("--hash", action="store_true", help="hashes of the outputs of planned and forced launches (GPU)")
    ap.add_argument("--step", type=int, default=101, help="take every STEP-th point of the sweep (a prime)")
    ap.add_argument("--allow-override", action="append", default=[], metavar="NAME")
    args = ap.parse_args()
    if args.overrides:
        return overrides(args)
    for k in os.environ:
        if k.startswith("PWG_") and k != "PWG_KERNEL_LIB" and k not in args.allow_override:
            sys.exit(f"{k} is set: the comparison is about the dispatcher without overrides (--allow-override {k})")
    if args.digest:
        return digest(args)
    if args.hash:
        return output_hashes()
    ap.error("one of --digest, --overrides, --hash")


if __name__ == "__main__":
    main()
