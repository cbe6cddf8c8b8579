"""Isolated A/B of the split-operand residual unit (csrc/resunit_split.hip) against the incumbents of its class on the
residual units of the last two stages of HiFi-GAN V1 (C = 64 at T = 128 F, C = 32 at T = 256 F), alternating in one
process.  GPU box only.
usage: bench_resunit_split.py [--json FILE] B F [B F ...]   -> one table per (utterances, mel frames); FILE: the rows as JSON
       bench_resunit_split.py --only-unit C K D B T  -> three launches of the new kernel on one class (counter passes)
Candidates per class (pair form, both biases): unit_fp32 = the one-launch fp32 unit (csrc/resunit.hip), 2xfp32 = two
fp32 convolutions, 2xsplit = two general split-operand launches, unit16 / unit32 = the new unit at the 16x16x32 /
32x32x16 bf16 MFMA.  The incumbent is what the forward runs today: 2xfp32 at C = 64, k = 11 (pwg_resunit_profitable
refuses that class), unit_fp32 elsewhere.  Per class: median and min..max of ROUNDS timed runs of each candidate, the
speed-up of the better new form over the incumbent, whether their ranges are disjoint, and the largest difference of
the two outputs relative to the largest output magnitude."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from parallelwavegan_amd import ops

ROUNDS, REPS = 5, 5
SLOPE = 0.1


def timeit(fn, reps=REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # us


def operands(ch, k, d, B, T):
    dev = torch.device("cuda:0")
    pad = (k - 1) // 2
    o = dict(x=torch.randn(B, ch, T, device=dev), b1=torch.randn(ch, device=dev), b2=torch.randn(ch, device=dev),
             h=torch.empty(B, ch, T, device=dev), y=torch.empty(B, ch, T, device=dev))
    w1, w2 = torch.randn(ch, ch, k, device=dev) * 0.05, torch.randn(ch, ch, k, device=dev) * 0.05
    o["d1"] = ops.make_conv_desc(B, ch, ch, T, T, k, dilation=d, pad_left=pad * d, pre_act="leaky_relu", pre_slope=SLOPE,
                                 post_act="leaky_relu", post_slope=SLOPE)
    o["d2"] = ops.make_conv_desc(B, ch, ch, T, T, k, dilation=1, pad_left=pad)
    o["unit"] = ops.make_resunit_desc(B, ch, T, k, d, True, SLOPE, SLOPE, 1.0)
    o["p1"], o["p2"] = ops.pack_weight(o["d1"], w1), ops.pack_weight(o["d2"], w2)
    o["s1"], o["s2"] = ops.pack_weight_split(o["d1"], w1), ops.pack_weight_split(o["d2"], w2)
    o["r1"], o["r2"] = ops.resunit_pack_weight(w1), ops.resunit_pack_weight(w2)
    return o


def candidates(o):
    x, h, y, b1, b2 = o["x"], o["h"], o["y"], o["b1"], o["b2"]

    def two_fp32():
        ops.conv1d_forward(o["d1"], x, o["p1"], b1, out=h)
        return ops.conv1d_forward(o["d2"], h, o["p2"], b2, x, out=y)

    def two_split():
        ops.conv1d_forward_split(o["d1"], x, o["s1"], b1, out=h)
        return ops.conv1d_forward_split(o["d2"], h, o["s2"], b2, x, out=y)

    runs = {}
    if ops.resunit_supported(o["unit"]):
        runs["unit_fp32"] = lambda: ops.resunit_forward(o["unit"], x, o["r1"], b1, o["r2"], b2, out=y)
    runs["2xfp32"] = two_fp32
    if ops.conv1d_split_supported(o["d1"]) and ops.conv1d_split_supported(o["d2"]):
        runs["2xsplit"] = two_split
    if ops.resunit_split_supported(o["unit"]):
        for shape in (16, 32):
            runs[f"unit{shape}"] = (lambda s: lambda: ops.resunit_forward_split(o["unit"], x, o["s1"], b1, o["s2"], b2,
                                                                                out=y, mfma_shape=s))(shape)
    return runs


def table(B, F, rows):
    print(f"# B = {B}, F = {F}: us per unit, median [min .. max] of {ROUNDS} rounds x {REPS} launches, alternating")
    for ch, T in ((64, F * 128), (32, F * 256)):
        for k in (3, 7, 11):
            for d in (1, 5):
                o = operands(ch, k, d, B, T)
                runs = candidates(o)
                incumbent = "unit_fp32" if ops.resunit_profitable(o["unit"]) else "2xfp32"
                if "unit16" not in runs:
                    print(f"unit {ch:3d} k{k:<2d} d{d} T={T:7d} not covered by the split unit")
                    continue
                ref = runs[incumbent]().clone()
                diff = ((runs["unit16"]() - ref).abs().max() / ref.abs().max()).item()
                for fn in runs.values():
                    fn()
                ts = {n: [] for n in runs}
                for _ in range(ROUNDS):
                    for n, fn in runs.items():
                        ts[n].append(timeit(fn))
                med = {n: statistics.median(v) for n, v in ts.items()}
                best = min(("unit16", "unit32"), key=lambda n: med[n])
                disjoint = max(ts[best]) < min(ts[incumbent])
                flops = 2 * 2.0 * ch * ch * k * T * B
                cells = "  ".join(f"{n} {med[n]:8.1f} [{min(ts[n]):8.1f} .. {max(ts[n]):8.1f}]" for n in runs)
                print(f"unit {ch:3d} k{k:<2d} d{d} T={T:7d} {cells}  {best} vs {incumbent} {med[incumbent] / med[best]:5.2f}x "
                      f"{'disjoint' if disjoint else 'overlap '} {flops / med[best] / 1e6:6.1f} TF-equiv  diff {diff:.1e}",
                      flush=True)
                rows.append(dict(B=B, F=F, channels=ch, kernel=k, dilation=d, T=T, incumbent=incumbent, best=best,
                                 us=ts, diff=diff))


def launch_only(ch, k, d, B, T, reps=3):
    """A few launches of the new kernel alone on one class (the program of a counter pass)."""
    o = operands(ch, k, d, B, T)
    for _ in range(reps):
        ops.resunit_forward_split(o["unit"], o["x"], o["s1"], o["b1"], o["s2"], o["b2"], out=o["y"])
    torch.cuda.synchronize()


if __name__ == "__main__":
    if sys.argv[1:2] == ["--only-unit"]:  # --only-unit C K D B T
        launch_only(*[int(a) for a in sys.argv[2:7]])
        sys.exit(0)
    argv, out = sys.argv[1:], None
    if argv[:1] == ["--json"]:
        out, argv = argv[1], argv[2:]
    args = [int(a) for a in argv] or [16, 800]
    rows = []
    for i in range(0, len(args), 2):
        table(args[i], args[i + 1], rows)
    if out:
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)
