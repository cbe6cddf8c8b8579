"""Host sweep of ``ops.conv1d_wgrad_plan`` (no GPU): which variants of conv1d_wgrad_kernel can the dispatcher select
without environment overrides?  Sweeps k 1..41, stride 1..13, dilation 1..512 and width 1..40 on a wide layer
(128 -> 128 channels: the 64 x 64 tile unless the LDS forces the second pass) and a narrow one (32 -> 32: the 32 x 32
tile), plain and pre-activated, and prints every distinct value of the plan's variant keys with one geometry that
reaches it.  tests/wgrad_cases.py takes its required (small, tg) set from this output.

Limits: one wide and one narrow layer (groups 1, no padding, --rows output rows, --batch items), the plain entry point
only -- tile, taps per wave, chunk length, windows, MODE, activation and stride instantiation depend on nothing else; the
number of slices and the finisher (which also depend on batch, length and weight norm) are not swept, the table pins them
case by case.  The full sweep is 43.7 million queries from Python: about 4 minutes on one core; --max-dilation 64
--max-width 8 (11 seconds) already shows every (small, tg).

--digest: one sha256 over the dispatcher's answers instead of the table, to show that two builds of the library
(PWG_KERNEL_LIB names another one) decide alike.  Hashed in a fixed order: the status code of every query and, where it is
0, all 20 integers (out[] is not cleared on a refusal) -- every case of tests/wgrad_cases.py under its own concurrency hint
with weight_norm 0 / 1 x has_bias 0 / 1 plus both workspace queries, then the sweep with weight_norm 0 and 1.

Usage: python tools/sweep_wgrad_plan.py [--max-dilation 512] [--max-width 40] [--digest]
"""
import argparse
import ctypes
import hashlib
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from parallelwavegan_amd import _lib, ops  # noqa: E402

from tests import wgrad_cases  # noqa: E402
from tests.wgrad_cases import OVERRIDE_PREFIXES as OVERRIDES  # noqa: E402


def sweep(args):
    """(geometry, descriptor) of every point of the sweep."""
    for chans in (128, 32):
        for width in range(1, args.max_width + 1):
            for k in range(1, 42):
                for stride in range(1, 14):
                    for dil in range(1, args.max_dilation + 1):
                        t_out = args.rows
                        t_in = (t_out - 1) * stride + (k - 1) * dil + 1
                        for pre in (None, "leaky_relu"):
                            yield (f"C{chans} W{width} k{k} s{stride} d{dil} pre={pre}",
                                   ops.make_conv_desc(args.batch, chans, chans, t_in, t_out, k, stride, dil, 0, 1, width=width,
                                                      pre_act=pre, pre_slope=0.1))


def digest(args):
    lib = _lib.lib()
    fn = lib.pwg_conv1d_backward_weight_plan
    out = (ctypes.c_int32 * 20)()
    h = hashlib.sha256()
    total = refused = 0

    def ask(d, wn, bias):
        nonlocal total, refused
        rc = fn(ctypes.byref(d), wn, bias, out)
        total += 1
        refused += rc != 0
        h.update(struct.pack("<i", rc))
        if rc == 0:
            h.update(bytes(out))

    for case in wgrad_cases.CASES:
        d = wgrad_cases.make_desc(case)
        with wgrad_cases.concurrency_hint(case["hint"]):
            for wn in (0, 1):
                for bias in (0, 1):
                    ask(d, wn, bias)
            h.update(struct.pack("<QQ", lib.pwg_conv1d_backward_weight_workspace_floats(ctypes.byref(d)),
                                 lib.pwg_conv1d_backward_weight_wn_workspace_floats(ctypes.byref(d))))
    for _, d in sweep(args):
        ask(d, 0, 1)
        ask(d, 1, 1)
    print(f"{_lib.LIB_PATH}: {total} queries, {refused} refused, --max-dilation {args.max_dilation} --max-width "
          f"{args.max_width} --rows {args.rows} --batch {args.batch}")
    print("sha256 " + h.hexdigest())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-dilation", type=int, default=512)
    ap.add_argument("--max-width", type=int, default=40)
    ap.add_argument("--rows", type=int, default=96, help="output rows (t_out) per item")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--digest", action="store_true", help="print one hash of every answer instead of the table")
    args = ap.parse_args()
    for k in os.environ:
        if k.startswith(OVERRIDES):
            sys.exit(f"{k} is set: the sweep is about the dispatcher without overrides")
    if args.digest:
        return digest(args)
    fn = _lib.lib().pwg_conv1d_backward_weight_plan
    out = (ctypes.c_int32 * 20)()
    seen = {}       # (key, value) -> first geometry
    refused = 0
    total = 0
    for geo, d in sweep(args):
        total += 1
        if fn(ctypes.byref(d), 0, 1, out) != 0:
            refused += 1
            continue
        if out[0] != 0:
            continue
        small, tg, win, tt, x4, mode, act, sct = out[4], out[5], out[8], out[9], out[11], out[12], out[13], out[14]
        for key in ((("small", small), ("tg", tg)), (("small", small), ("tt", tt), ("mode", mode)),
                    (("small", small), ("mode", mode), ("act", act), ("win", win)),
                    (("mode", mode), ("act", act), ("stride_ct", sct)), (("mode", mode), ("rows_x4", x4))):
            seen.setdefault(key, geo)
    print(f"{total} descriptors, {refused} refused (more than 160 KiB of LDS)")
    for key in sorted(seen):
        print("  " + " ".join(f"{n}={v}" for n, v in key) + "   e.g. " + seen[key])
    print("reachable (small, tg):", sorted({(dict(k)["small"], dict(k)["tg"]) for k in seen if dict(k).keys() == {"small", "tg"}}))


if __name__ == "__main__":
    main()
