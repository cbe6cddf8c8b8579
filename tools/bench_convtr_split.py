"""Isolated-layer A/B of the split-operand transposed kernel (csrc/conv1d_split.hip, convtr1d_split_mfma_kernel) against
the fp32 kernel on the four upsampling layers of HiFi-GAN V1, with the one-product bf16 kernel as a staging-bound
yardstick, alternating in one process.  GPU box only.
usage: bench_convtr_split.py B F [B F ...]          -> one table per (utterances, mel frames)
       bench_convtr_split.py --only-split CIN COUT S B T_IN   -> three launches of the new kernel on one class (counter passes)
Per class: median and min..max of ROUNDS timed runs of each kernel, the speed-up of the medians over the fp32 kernel,
whether the two ranges are disjoint, and the largest difference of the two outputs relative to the largest magnitude."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from parallelwavegan_amd import ops
from tools.bench_conv_split import REPS, ROUNDS, timeit

LAYERS = ((512, 256, 8), (256, 128, 8), (128, 64, 2), (64, 32, 2))  # (c_in, c_out, stride), kernel = 2 * stride


def _layer(cin, cout, s, B, T, dev):
    t_out = ops.conv_transpose_out_length(T, 2 * s, s, s // 2, 0)
    desc = ops.make_conv_desc(B, cin, cout, T, t_out, 2 * s, s, 1, s // 2, transposed=True, pre_act="leaky_relu",
                              pre_slope=0.1)
    w = torch.randn(cin, cout, 2 * s, device=dev) * 0.05
    x, bias = torch.randn(B, cin, T, device=dev), torch.randn(cout, device=dev)
    return desc, w, x, bias, torch.empty(B, cout, t_out, device=dev)


def table(B, F):
    dev = torch.device("cuda:0")
    print(f"# B = {B}, F = {F}: us per launch, median [min .. max] of {ROUNDS} rounds x {REPS} launches, alternating")
    T = F
    for cin, cout, s in LAYERS:
        desc, w, x, bias, y = _layer(cin, cout, s, B, T, dev)
        wp, wb, ws = ops.pack_weight(desc, w), ops.pack_weight_bf16(desc, w), ops.pack_weight_split_transposed(desc, w)
        runs = {
            "fp32": lambda: ops.conv1d_forward(desc, x, wp, bias, out=y),
            "bf16": lambda: ops.conv1d_forward_bf16(desc, x, wb, bias, out=y),
            "split16": lambda: ops.conv1d_forward_split_transposed(desc, x, ws, bias, out=y, mfma_shape=16),
            "split32": lambda: ops.conv1d_forward_split_transposed(desc, x, ws, bias, out=y, mfma_shape=32),
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
        cells = "  ".join(f"{n} {med[n]:7.1f} [{min(ts[n]):7.1f} .. {max(ts[n]):7.1f}]" for n in runs)
        flops = 2.0 * B * cin * cout * 2 * s * T
        print(f"up {cin:3d}->{cout:3d} s{s} cols={B * desc.t_out:8d} {cells}  {best} {med['fp32'] / med[best]:5.2f}x "
              f"{'disjoint' if max(ts[best]) < min(ts['fp32']) else 'overlap '}  "
              f"split16 {med['fp32'] / med['split16']:5.2f}x {'disjoint' if max(ts['split16']) < min(ts['fp32']) else 'overlap '} "
              f"{flops / med[best] / 1e6:6.1f} TF-equiv  diff {diff:.1e}", flush=True)
        T *= s


def launch_only(cin, cout, s, B, T, reps=3):
    """A few launches of the new kernel alone on one class (the program of a counter pass)."""
    dev = torch.device("cuda:0")
    desc, w, x, bias, y = _layer(cin, cout, s, B, T, dev)
    ws = ops.pack_weight_split_transposed(desc, w)
    for _ in range(reps):
        ops.conv1d_forward_split_transposed(desc, x, ws, bias, out=y)
    torch.cuda.synchronize()


if __name__ == "__main__":
    if sys.argv[1:2] == ["--only-split"]:
        launch_only(*[int(a) for a in sys.argv[2:7]])
        sys.exit(0)
    args = [int(a) for a in sys.argv[1:]] or [16, 800]
    for i in range(0, len(args), 2):
        table(args[i], args[i + 1])
