"""Isolated A/B of the chained block of split-operand residual units (resblock_split_kernel, csrc/resunit_split.hip)
against the N one-launch units it replaces, as the forward routes them today (ops.resunit_forward_split at its default
MFMA shape), on the residual blocks of the last two stages of HiFi-GAN V1 (C = 64 at T = 128 F, C = 32 at T = 256 F),
alternating in one process.  GPU box only.
usage: bench_resblock_split.py [--json FILE] B F [B F ...]   -> one table per (utterances, mel frames); FILE: the rows as JSON
       bench_resblock_split.py --only-block C K N B T  -> three launches of the block alone on one class (counter passes)
Classes: (C, k) in {32, 64} x {3, 7} and (32, 11), N = 3 (dilations 1, 3, 5; with the MRF addend where k != 3, as in the
forward) and N = 2 (dilations 1, 3, no addend: the block in front of a pending join).  Per class: median and min..max of
ROUNDS timed runs of REPS launches each, after WARM untimed rounds; the speed-up; whether the ranges are disjoint;
whether the outputs are equal to the bit."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from parallelwavegan_amd import _lib, ops

WARM, ROUNDS, REPS = 3, 7, 5
SLOPE = 0.1
DILATIONS = (1, 3, 5)
CLASSES = [(32, 3), (32, 7), (32, 11), (64, 3), (64, 7)]


def timeit(fn, reps=REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # us


def operands(ch, k, n, B, T, addend):
    dev = torch.device("cuda:0")
    wdesc = ops.make_conv_desc(1, ch, ch, 64, 64, k, pad_left=(k - 1) // 2)
    o = dict(x=torch.randn(B, ch, T, device=dev), add2=torch.randn(B, ch, T, device=dev) if addend else None,
             y=[torch.empty(B, ch, T, device=dev) for _ in range(n)], yb=torch.empty(B, ch, T, device=dev),
             b1=[torch.randn(ch, device=dev) for _ in range(n)], b2=[torch.randn(ch, device=dev) for _ in range(n)],
             s1=[ops.pack_weight_split(wdesc, torch.randn(ch, ch, k, device=dev) * 0.05) for _ in range(n)],
             s2=[ops.pack_weight_split(wdesc, torch.randn(ch, ch, k, device=dev) * 0.05) for _ in range(n)])
    o["units"] = [ops.make_resunit_desc(B, ch, T, k, DILATIONS[u], True, SLOPE, SLOPE, 1.0) for u in range(n)]
    return o


def candidates(o, n):
    def units():
        x = o["x"]
        for u in range(n):
            x = ops.resunit_forward_split(o["units"][u], x, o["s1"][u], o["b1"][u], o["s2"][u], o["b2"][u],
                                          o["add2"] if u == n - 1 else None, out=o["y"][u])
        return x

    def block():
        return ops.resblock_forward_split(o["units"][0], o["x"], DILATIONS[:n], (SLOPE,) * n, (SLOPE,) * n, o["s1"],
                                          o["b1"], o["s2"], o["b2"], o["add2"], out=o["yb"])

    return {"units": units, "block": block}


def table(B, F, rows):
    print(f"# B = {B}, F = {F}: us per block, median [min .. max] of {ROUNDS} rounds x {REPS} launches, alternating")
    for ch, k in CLASSES:
        T = F * (128 if ch == 64 else 256)
        for n in (3, 2):
            desc = ops.make_resunit_desc(B, ch, T, k, 1, True, SLOPE, SLOPE, 1.0)
            if not ops.resblock_split_supported(desc, DILATIONS[:n]):
                print(f"block {ch:3d} k{k:<2d} N{n} T={T:7d} refused: {_lib.lib().pwg_last_error().decode()}")
                continue
            o = operands(ch, k, n, B, T, addend=(n == 3 and k != 3))
            runs = candidates(o, n)
            same = torch.equal(runs["units"](), runs["block"]())
            for _ in range(WARM):
                for fn in runs.values():
                    timeit(fn)
            ts = {name: [] for name in runs}
            for _ in range(ROUNDS):
                for name, fn in runs.items():
                    ts[name].append(timeit(fn))
            med = {name: statistics.median(v) for name, v in ts.items()}
            wins, loses = max(ts["block"]) < min(ts["units"]), min(ts["block"]) > max(ts["units"])
            cells = "  ".join(f"{name} {med[name]:8.1f} [{min(ts[name]):8.1f} .. {max(ts[name]):8.1f}]" for name in runs)
            print(f"block {ch:3d} k{k:<2d} N{n} T={T:7d} {cells}  {med['units'] / med['block']:5.2f}x "
                  f"{'block wins, disjoint' if wins else 'block loses, disjoint' if loses else 'overlap'}  "
                  f"{'equal bits' if same else 'BITS DIFFER'}", flush=True)
            rows.append(dict(B=B, F=F, channels=ch, kernel=k, n_units=n, T=T, us=ts, equal=same))


def launch_only(ch, k, n, B, T, reps=3):
    """A few launches of the block alone on one class (the program of a counter pass)."""
    o = operands(ch, k, n, B, T, addend=False)
    block = candidates(o, n)["block"]
    for _ in range(reps):
        block()
    torch.cuda.synchronize()


if __name__ == "__main__":
    if sys.argv[1:2] == ["--only-block"]:  # --only-block C K N B T
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
