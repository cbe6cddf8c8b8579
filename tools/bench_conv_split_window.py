"""Isolated A/B of the two forms of the split-operand kernel's window staging (csrc/conv1d_split.hip: staged =
``conv1d_split_mfma_kernel``, prefetched = ``conv1d_split_window_mfma_kernel``) on the few-tap classes of the HiFi-GAN V1
forward: the 256- and 128-channel k = 3 residual convolutions at dilations 1 / 3 / 5, each at the length of its stage;
with ``--all`` also, for information, k = 7 / 11 and the 64-channel pairs.  Both forms run the resident step and are
launched from ONE library through ``pwg_conv1d_split_forward_window``, alternating in one process with the fp32 kernel
(``conv1d_mfma_dma_kernel``, the incumbent of these classes) and, for information, the staged window with the streamed
step, after WARMUP untimed rounds per class.  GPU box only.
usage: bench_conv_split_window.py [--all] [--json FILE] B F [B F ...]   -> one table per (utterances, mel frames)
       bench_conv_split_window.py --only FORM C K D B T   -> three launches of one form (1 / 2) on one class (counter passes)
Per class: median and min..max of ROUNDS timed runs of each candidate, staged / prefetched of the medians, whether the
two ranges are disjoint ("faster" / "slower": every prefetched run below / above every staged run), fp32 / the plan's
form and whether that is disjoint, what the launch plan chooses, and whether the two outputs are the same bits.  The
keep rule of DESIGN.md s9.1 reads this table: a class is admitted to the prefetched form when it is "faster" at 16 x 800
and "slower" at no shorter launch."""
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
RESIDENT, STREAMED = 1, 2


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
    desc = ops.make_conv_desc(B, ch, ch, T, T, k, dilation=d, pad_left=(k - 1) // 2 * d, pre_act="leaky_relu",
                              pre_slope=0.1)
    torch.manual_seed(ch + k + d)
    w = torch.randn(ch, ch, k, device=dev) * 0.05
    return dict(desc=desc, wp=ops.pack_weight(desc, w), ws=ops.pack_weight_split(desc, w),
                x=torch.randn(B, ch, T, device=dev), bias=torch.randn(ch, device=dev),
                add1=torch.randn(B, ch, T, device=dev), y=torch.empty(B, ch, T, device=dev))


def table(B, F, rows, everything):
    print(f"# B = {B}, F = {F}: us per launch, median [min .. max] of {ROUNDS} rounds x {REPS} launches, alternating")
    classes = [(ch, up, 3, d) for ch, up in STAGES[:2] for d in (1, 3, 5)]
    if everything:
        classes += [(ch, up, k, d) for ch, up in STAGES for k in (7, 11) for d in (1, 5)]
        classes += [(64, 128, 3, d) for d in (1, 5)]
    for ch, up, k, d in classes:
        T = F * up
        o = operands(ch, k, d, B, T)
        desc, x, bias, add1, y = o["desc"], o["x"], o["bias"], o["add1"], o["y"]
        runs = {name: (lambda f: lambda: ops.conv1d_forward_split(desc, x, o["ws"], bias, add1, out=y,
                                                                  step_form=RESIDENT, window_form=f))(f)
                for f, name in ops.WINDOW_FORMS.items()}
        same = torch.equal(runs["staged"]().clone(), runs["prefetched"]())
        # for information: the staged window with the streamed step, which the plan keeps for k >= 7
        runs["streamed"] = lambda: ops.conv1d_forward_split(desc, x, o["ws"], bias, add1, out=y, step_form=STREAMED,
                                                            window_form=1)
        runs["fp32"] = lambda: ops.conv1d_forward(desc, x, o["wp"], bias, add1, out=y)
        for _ in range(WARMUP):  # new tensors, new kernels: the first rounds of a class are not its steady state
            for fn in runs.values():
                timeit(fn)
        ts = {n: [] for n in runs}
        for _ in range(ROUNDS):
            for n, fn in runs.items():
                ts[n].append(timeit(fn))
        med = {n: statistics.median(v) for n, v in ts.items()}
        verdict = ("faster" if max(ts["prefetched"]) < min(ts["staged"]) else
                   "slower" if min(ts["prefetched"]) > max(ts["staged"]) else "overlap")
        plan = ops.conv1d_split_window_form(desc)
        vs_fp32 = "disjoint" if max(ts[plan]) < min(ts["fp32"]) else "overlap "
        cells = "  ".join(f"{n} {med[n]:8.1f} [{min(ts[n]):8.1f} .. {max(ts[n]):8.1f}]" for n in runs)
        print(f"conv {ch:3d} k{k:<2d} d{d} T={T:7d} {cells}  {med['staged'] / med['prefetched']:5.3f}x {verdict:7s} "
              f"plan {plan}  fp32/plan {med['fp32'] / med[plan]:5.2f}x {vs_fp32}  "
              f"{'same bits' if same else 'BITS DIFFER'}", flush=True)
        rows.append(dict(B=B, F=F, channels=ch, kernel=k, dilation=d, T=T, us=ts, verdict=verdict, plan=plan,
                         same_bits=same))


def launch_only(form, ch, k, d, B, T, reps=3):
    """A few launches of one form alone on one class (the program of a counter pass)."""
    o = operands(ch, k, d, B, T)
    for _ in range(reps):
        ops.conv1d_forward_split(o["desc"], o["x"], o["ws"], o["bias"], o["add1"], out=o["y"], step_form=RESIDENT,
                                 window_form=form)
    torch.cuda.synchronize()


if __name__ == "__main__":
    argv, out, everything = sys.argv[1:], None, False
    if argv[:1] == ["--only"]:  # --only FORM C K D B T
        launch_only(*[int(a) for a in argv[1:7]])
        sys.exit(0)
    if argv[:1] == ["--all"]:
        everything, argv = True, argv[1:]
    if argv[:1] == ["--json"]:
        out, argv = argv[1], argv[2:]
    args = [int(a) for a in argv] or [16, 800]
    rows = []
    for i in range(0, len(args), 2):
        table(args[i], args[i + 1], rows, everything)
    if out:
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)
