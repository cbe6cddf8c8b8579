"""Isolated-layer A/B of the split-operand kernel (csrc/conv1d_split.hip) against the fp32 kernel on the residual
convolutions of HiFi-GAN V1 (the rows of tools/bench_conv.py), alternating in one process.  GPU box only.
usage: bench_conv_split.py B F [B F ...]     -> one table per (utterances, mel frames)
       bench_conv_split.py --only-split C K D B T   -> three launches of the split kernel on one class (counter passes)
Per class: median and min..max of ROUNDS timed runs of each kernel, the speed-up of the medians, whether the two ranges
are disjoint, and the largest difference of the two outputs relative to the largest output magnitude."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from parallelwavegan_amd import ops

ROUNDS, REPS = 5, 5


def timeit(fn, reps=REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # us


def table(B, F):
    dev = torch.device("cuda:0")
    print(f"# B = {B}, F = {F}: us per launch, median [min .. max] of {ROUNDS} rounds x {REPS} launches, alternating")
    ch, T = 512, F
    for s in (8, 8, 2, 2):
        ch //= 2
        T *= s
        for k in (3, 7, 11):
            for d in (1, 5):
                desc = ops.make_conv_desc(B, ch, ch, T, T, k, dilation=d, pad_left=(k - 1) // 2 * d,
                                          pre_act="leaky_relu", pre_slope=0.1)
                if not ops.conv1d_split_supported(desc):
                    print(f"res {ch:3d} k{k:<2d} d{d} T={T:7d} not covered by the split kernel")
                    continue
                w = torch.randn(ch, ch, k, device=dev) * 0.05
                x = torch.randn(B, ch, T, device=dev)
                bias = torch.randn(ch, device=dev)
                add1 = torch.randn(B, ch, T, device=dev)
                y = torch.empty(B, ch, T, device=dev)
                wp, ws = ops.pack_weight(desc, w), ops.pack_weight_split(desc, w)
                runs = {
                    "fp32": lambda: ops.conv1d_forward(desc, x, wp, bias, add1, out=y),
                    "split16": lambda: ops.conv1d_forward_split(desc, x, ws, bias, add1, out=y, mfma_shape=16),
                    "split32": lambda: ops.conv1d_forward_split(desc, x, ws, bias, add1, out=y, mfma_shape=32),
                }
                ref = runs["fp32"]().clone()
                diff = ((runs["split16"]() - ref).abs().max() / ref.abs().max()).item()
                for fn in runs.values():
                    fn()
                ts = {n: [] for n in runs}
                for _ in range(ROUNDS):
                    for n, fn in runs.items():
                        ts[n].append(timeit(fn))
                med = {n: statistics.median(v) for n, v in ts.items()}
                best = min(("split16", "split32"), key=lambda n: med[n])
                disjoint = max(ts[best]) < min(ts["fp32"])
                flops = 2.0 * ch * ch * k * T * B
                cells = "  ".join(f"{n} {med[n]:8.1f} [{min(ts[n]):8.1f} .. {max(ts[n]):8.1f}]" for n in runs)
                print(f"res {ch:3d} k{k:<2d} d{d} T={T:7d} {cells}  {best} {med['fp32'] / med[best]:5.2f}x "
                      f"{'disjoint' if disjoint else 'overlap '} {flops / med[best] / 1e6:6.1f} TF-equiv  "
                      f"diff {diff:.1e}", flush=True)


def launch_only(ch, k, d, B, T, reps=3):
    """A few launches of the split kernel alone on one class (the program of a counter pass)."""
    dev = torch.device("cuda:0")
    desc = ops.make_conv_desc(B, ch, ch, T, T, k, dilation=d, pad_left=(k - 1) // 2 * d, pre_act="leaky_relu", pre_slope=0.1)
    ws = ops.pack_weight_split(desc, torch.randn(ch, ch, k, device=dev) * 0.05)
    x, bias, add1 = torch.randn(B, ch, T, device=dev), torch.randn(ch, device=dev), torch.randn(B, ch, T, device=dev)
    y = torch.empty(B, ch, T, device=dev)
    for _ in range(reps):
        ops.conv1d_forward_split(desc, x, ws, bias, add1, out=y)
    torch.cuda.synchronize()


if __name__ == "__main__":
    if sys.argv[1:2] == ["--only-split"]:  # --only-split C K D B T
        launch_only(*[int(a) for a in sys.argv[2:7]])
        sys.exit(0)
    args = [int(a) for a in sys.argv[1:]] or [16, 800]
    for i in range(0, len(args), 2):
        table(args[i], args[i + 1])
