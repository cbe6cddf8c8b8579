"""Isolated A/B of the two forms of the split-operand kernel's reduction step (csrc/conv1d_split.hip: resident =
``conv1d_split_mfma_kernel``, streamed = ``conv1d_split_streamed_mfma_kernel``) on the classes the HiFi-GAN V1 forward
sends to the kernel: the 256- and 128-channel k = 7 / 11 residual convolutions and the 64-channel k = 7 / 11 pairs, each
at the length of its stage.  Both forms are launched from ONE library through ``pwg_conv1d_split_forward_step``,
alternating in one process, after WARMUP untimed rounds per class.  GPU box only.
usage: bench_conv_split_forms.py [--json FILE] B F [B F ...]   -> one table per (utterances, mel frames)
Per class: median and min..max of ROUNDS timed runs of each form, resident / streamed of the medians, whether the two
ranges are disjoint ("faster" / "slower": every streamed run below / above every resident run), what the launch plan
chooses, and whether the two outputs are the same bits.  The keep rule of DESIGN.md s9.1 reads this table: a class is
admitted to the streamed form when it is "faster" at 16 x 800 and "slower" at no shorter launch."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from parallelwavegan_amd import ops

ROUNDS, REPS, WARMUP = 7, 5, 3
# channels, samples per mel frame at the stage
STAGES = ((256, 8), (128, 64), (64, 128))


def timeit(fn, reps=REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # us


def table(B, F, rows):
    dev = torch.device("cuda:0")
    print(f"# B = {B}, F = {F}: us per launch, median [min .. max] of {ROUNDS} rounds x {REPS} launches, alternating")
    for ch, up in STAGES:
        T = F * up
        for k in (7, 11):
            for d in (1, 5):
                desc = ops.make_conv_desc(B, ch, ch, T, T, k, dilation=d, pad_left=(k - 1) // 2 * d,
                                          pre_act="leaky_relu", pre_slope=0.1)
                torch.manual_seed(ch + k + d)
                ws = ops.pack_weight_split(desc, torch.randn(ch, ch, k, device=dev) * 0.05)
                x, bias = torch.randn(B, ch, T, device=dev), torch.randn(ch, device=dev)
                add1 = torch.randn(B, ch, T, device=dev)
                y = torch.empty(B, ch, T, device=dev)
                runs = {name: (lambda f: lambda: ops.conv1d_forward_split(desc, x, ws, bias, add1, out=y, step_form=f))(f)
                        for f, name in ops.STEP_FORMS.items()}
                same = torch.equal(runs["resident"]().clone(), runs["streamed"]())
                for _ in range(WARMUP):  # new tensors, new kernels: the first rounds of a class are not its steady state
                    for fn in runs.values():
                        timeit(fn)
                ts = {n: [] for n in runs}
                for _ in range(ROUNDS):
                    for n, fn in runs.items():
                        ts[n].append(timeit(fn))
                med = {n: statistics.median(v) for n, v in ts.items()}
                verdict = ("faster" if max(ts["streamed"]) < min(ts["resident"]) else
                           "slower" if min(ts["streamed"]) > max(ts["resident"]) else "overlap")
                plan = ops.conv1d_split_step_form(desc)
                cells = "  ".join(f"{n} {med[n]:8.1f} [{min(ts[n]):8.1f} .. {max(ts[n]):8.1f}]" for n in runs)
                print(f"conv {ch:3d} k{k:<2d} d{d} T={T:7d} {cells}  {med['resident'] / med['streamed']:5.3f}x {verdict:7s} "
                      f"plan {plan}  {'same bits' if same else 'BITS DIFFER'}", flush=True)
                rows.append(dict(B=B, F=F, channels=ch, kernel=k, dilation=d, T=T, us=ts, verdict=verdict, plan=plan,
                                 same_bits=same))


if __name__ == "__main__":
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
